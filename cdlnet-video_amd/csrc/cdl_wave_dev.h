// Device-side pieces shared by the fused kernels (cdl_fused2d.hip, cdl_fusedg.hip, cdl_strip.hip, cdl_stripg.hip) and by
// the sparse matrix-core tier (cdl_analysis_mfma.hip, cdl_synth_mfma.hip, cdl_wgrad_mfma.hip).
// Included inside each file's anonymous namespace, so every object keeps its own internal copies.
#pragma once

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) unsigned u32x4;

constexpr int OOB = 0x7fff0000;              // byte offset beyond any buffer descriptor range: loads return 0, stores are dropped

enum { MODE_FWD = 0, MODE_FIRST = 1, MODE_BWD = 2 };

// Buffer descriptor from a WAVE-UNIFORM pointer.  hipcc cannot prove uniformity of anything derived from
// threadIdx (a wave index, an operator picked per wave group): it then wraps EVERY buffer access in a
// readfirstlane "waterfall" loop, which serialises the accesses (seen in k_wgrad2d: each of the 8-32 loads of
// a row block had its own loop; with bf16 storage each was followed by s_waitcnt vmcnt(0)).  Reading the
// pointer words through readfirstlane makes the descriptor provably scalar.
// SCALAR_SIZE: `bytes` is formed from kernel arguments alone, which hipcc does see as scalar, and is taken as it is (the
// sparse matrix-core tier: the readfirstlane of a scalar goes through a VGPR, which cost seven instances of k_ana_m and
// k_synth_m an occupancy step).
template <bool SCALAR_SIZE = false>
__device__ __forceinline__ __amdgpu_buffer_rsrc_t uniform_rsrc(const void *base, size_t bytes)
{
    const unsigned long long a = reinterpret_cast<unsigned long long>(base);
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)a);
    const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)(a >> 32));
    void *b = reinterpret_cast<void *>(((unsigned long long)hi << 32) | lo);
    return __builtin_amdgcn_make_buffer_rsrc(b, 0, SCALAR_SIZE ? (int)bytes : __builtin_amdgcn_readfirstlane((int)bytes), 0x00020000);
}

// v = hi + lo as two bf16 (round to nearest even, then the rounded remainder): the operand split of the split-bf16 products
__device__ __forceinline__ void split_bf16(float v, __bf16 &hi, __bf16 &lo)
{
    hi = (__bf16)v;
    lo = (__bf16)(v - (float)hi);
}
// the same for the 8 values of one MFMA operand fragment
__device__ __forceinline__ void split_bf16(const float (&v)[8], bf16x8 &hi, bf16x8 &lo)
{
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        __bf16 h, l;
        split_bf16(v[i], h, l);
        hi[i] = h;
        lo[i] = l;
    }
}

// acc += a b by three bf16 products of the parts, lo.hi, hi.lo, hi.hi in that order (split3: no lo.lo).  The order is part of
// the bits.  (k_ana_m issues the same three interleaved across its accumulator tiles and does not call this.)
__device__ __forceinline__ void mfma_split3(f32x16 &acc, const bf16x8 &ah, const bf16x8 &al, const bf16x8 &bh, const bf16x8 &bl)
{
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, acc, 0, 0, 0);
}

// ---- tap packing of the synthesis-like GEMM's M dimension (cdl_fusedg.hip, cdl_strip.hip, cdl_stripg.hip) ---------
// Row t of a 32-row accumulator tile sits in register v = 4*((t>>3)&3) + (t&3) of lane half h = (t>>2)&1.  The taps
// (i, j) of a P x P filter plane are assigned rows so that the column-direction col2im is a short static sequence:
// P = 3, 7: t = 8 i + j (as cdl_fused2d.hip); P = 5: 25 taps packed into ONE 32-row tile (8i + j would need two).
template <int P> __host__ __device__ constexpr int tap_slot(int i, int j)
{
    if (P == 5) return (i < 4 && j < 4) ? 8 * i + j : (i < 4 ? 8 * i + 4 : (j < 4 ? 8 * j + 5 : 6));
    return 8 * i + j;
}
template <int P> struct TapTiles { static constexpr int RT = (P == 7) ? 2 : 1; };     // 32-slot tap tiles

// lane i <- lane i-1 over the whole wave (lane 0 <- 0): one DPP modifier on the consuming add
__device__ __forceinline__ float wave_shr1(float v)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x138, 0xf, 0xf, true));
}
// lanes 0..31 receive the value held by lanes 32..63 (lanes 32..63 receive 0).
// v_permlane32_swap vdst, src exchanges vdst[32..63] with src[0..31]; with src = 0 the new src is
// {v.hi, 0}.  Inline asm because hipcc (ROCm 7.2) returns the SAME register for both results of
// __builtin_amdgcn_permlane32_swap (tools/probes/probe_dpp.hip); s_nop 1 = the two wait states the
// instruction needs after a VALU write of either operand.
__device__ __forceinline__ float upper_half_to_lower(float v)
{
    float lo = 0.0f;
    asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1\n\ts_nop 1" : "+v"(v), "+v"(lo));
    return lo;
}

// Sum over the 32 pixel lanes of each half-wave of N per-lane values, leaving total #i on lane
// (c with c mod N == i): a halving butterfly, N-1 exchanges instead of 5N.  Template recursion keeps
// every register index static.  (N = 16: lanes c and c ^ 16 end up with the two halves of total #(c mod 16).)
// DPP = true: the exchanges at distances 8, 4, 2 and 1 stay inside a 16-lane row and are DPP moves (lane_xor_dpp) instead of
// ds_bpermute round trips through LDS; longer distances keep __shfl_xor.  Same keep / send selection, same keep + received:
// the same bits.  Needs every lane of the wave active.
template <int DIST>
__device__ __forceinline__ float lane_xor_dpp(float v)
{
    static_assert(DIST == 8 || DIST == 4 || DIST == 2 || DIST == 1, "distances inside a 16-lane row");
    const int s = __builtin_bit_cast(int, v);
    int r;
    if constexpr (DIST == 8) {
        r = __builtin_amdgcn_update_dpp(0, s, 0x128, 0xf, 0xf, false);           // row_ror:8
    } else if constexpr (DIST == 4) {
        r = __builtin_amdgcn_update_dpp(0, s, 0x104, 0xf, 0x5, false);           // row_shl:4 (lane i <- i + 4) into banks 0, 2
        r = __builtin_amdgcn_update_dpp(r, s, 0x114, 0xf, 0xa, false);           // row_shr:4 (lane i <- i - 4) into banks 1, 3
    } else if constexpr (DIST == 2) {
        r = __builtin_amdgcn_update_dpp(0, s, 0x4e, 0xf, 0xf, false);            // quad_perm:[2,3,0,1]
    } else {
        r = __builtin_amdgcn_update_dpp(0, s, 0xb1, 0xf, 0xf, false);            // quad_perm:[1,0,3,2]
    }
    return __builtin_bit_cast(float, r);
}
template <int N, bool DPP = false>
struct LaneTransposeSum {
    static __device__ __forceinline__ float run(const float (&v)[N], int c)
    {
        constexpr int n = N / 2;
        const bool up = (c & n) != 0;
        float w[n];
#pragma unroll
        for (int k = 0; k < n; ++k) {
            const float keep = up ? v[k + n] : v[k];
            const float send = up ? v[k] : v[k + n];
            if constexpr (DPP && n <= 8) w[k] = keep + lane_xor_dpp<n>(send);
            else w[k] = keep + __shfl_xor(send, n, 64);
        }
        return LaneTransposeSum<n, DPP>::run(w, c);
    }
};
template <bool DPP>
struct LaneTransposeSum<1, DPP> {
    static __device__ __forceinline__ float run(const float (&v)[1], int) { return v[0]; }
};
