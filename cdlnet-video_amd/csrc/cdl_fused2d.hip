// Fused ISTA iteration for the flagship shape family (2-D, C = 1, stride 1, P <= 7,
// M = 32 or 64) on the gfx950 matrix cores.
//
// Fusion boundary.  The iteration z' = ST(z - A(mask*B z - yp), tau) is cut where the tensor is
// THIN (one channel), not where it is fat (M channels):
//
//     launch k :  r_k (thin) , z_k (fat)  ->  z_{k+1} (fat) , partial B_{k+1} z_{k+1} (thin patches)
//
// so every fat tensor crosses HBM exactly once in and once out per iteration and needs NO halo:
// z_k[pixel] is only used pointwise, the (P-1) halo lives on the one-channel residual r_k, which is
// tiny and L2 resident.  Inside the launch, per 32-pixel row block of a wave:
//
//   analysis   acc[ch][px]  = sum_k  W_A[ch][k] * im2col(r)[k][px]        MFMA 32x32x16 bf16, K = 64
//   epilogue   z'           = ST(z -/+ acc, tau)  -> global                (z loaded in the MFMA C/D layout)
//   synthesis  col[tap][px] = sum_ch W_B^T[tap][ch] * z'[ch][px]           MFMA, z' fed straight from the
//                                                                          accumulator registers (no LDS)
//   col2im     rsum[y-3+i][x-3+j] += col[(i,j)][y,x]                       row direction summed in registers
//                                                                          (7-row ring), column direction
//                                                                          through ds_add_f32
//
// fp32-grade accuracy on bf16 matrix cores: every operand is split v = hi + lo (two bf16) and each
// product is hi*hi + hi*lo + lo*hi with fp32 accumulation (relative error ~2^-16 per product, random
// sign; measured end-to-end parity is recorded in DESIGN.md).  PREC = 1 drops the lo terms (plain bf16).
//
// Work decomposition: workgroup = 256 threads = 4 waves, ONE per SIMD, = 64 x 16 pixel tile of one image (2 x 2 waves of
// 32 x 8); persistent grid, one workgroup per CU.  (Rounds 1-2: 8 waves on 64 x 32 tiles, two per SIMD so that a wave's memory
// waits were covered by its partner -- Shape<4> below is that form.  One wave per SIMD costs the forward nothing and the
// reverse stage 11 %, and frees the registers -- up to 512 per wave -- and the LDS that let the reverse stage accumulate
// dA_k itself: one fat pass per iteration less)  Weight fragments: staged through LDS (32 KB) once per
// workgroup, then resident in every wave's registers.  Each
// workgroup writes its (16+6) x (64+6) partial synthesis patch; k_assemble sums the <= 4 overlapping
// patches per pixel in a fixed order and applies mask / -yp.  Every reduction (col2im slabs, dtau,
// filter gradients) is combined in a fixed order: results are bit-reproducible run to run.
#include <atomic>
#include <cstdlib>
#include <type_traits>
#include <mutex>
#include <utility>
#include <vector>

#include "cdl_common.h"
#include "cdl_fused_sweep.h"

// Two tile shapes, one template argument.  Everything that works on the stage's tiles takes WY, the wave rows per workgroup
// (Shape<WY> below): WY = 2 is the shape described above and the one every step-wise entry point uses; WY = 4 is rounds
// 1-2's 64 x 32 tile with two waves per SIMD.  cdl_fused2d_forward / _backward run sweeps with bf16 code STORAGE
// (CDL_LAY_BLK16) on WY = 4: those kernels are compute-bound, and lose at one wave per SIMD what the fp32-storage sweep gains
// from it (28.5 against 26.5 ms/step).  Only the kernels such a sweep can launch exist at WY = 4 (launch_stage_lay).

namespace {

#include "cdl_wave_dev.h"

typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;

constexpr int WX = 2;                       // waves per workgroup along x
constexpr int RB = 8;                       // row blocks (image rows) per wave
constexpr int TW = 32 * WX;                 // tiles are 64 pixels wide
constexpr int HALO = 3;                     // filters are embedded in a 7 x 7 (padded 8 x 8) tap grid
constexpr int RTW = TW + 2 * HALO;          // 70 columns of residual tile / patch
constexpr int RTC = RTW + 2;                // columns kept in LDS (col 70 is the zero-weight pad tap)
constexpr int LDS_W = 32 * 64 * 16;         // 32 weight fragments of 1 KB (split3, M = 64)
constexpr int LDS_TAU = 64 * 4;

constexpr int GW_TH = 16;                    // tile rows of the filter-gradient kernel
constexpr int GW_RTH = GW_TH + 2 * HALO;     // 22
constexpr int TROWS = GW_RTH + 1;            // halo rows + the (never used) i = 7 pad row
constexpr int TPITCH = 72;                   // bf16 elements per row of a shifted copy (144 B)
constexpr int TCOPY = TROWS * TPITCH;
constexpr int WG_THIN_BYTES = 2 * 2 * 4 * TCOPY * 2;      // [op][hl][shift] copies               (52992)
constexpr int IMG_ELEMS = 32 * 32;           // one [32 px][32 ch] bf16 image (2 KB)

// What depends on the tile height.  WY_ = wave rows per workgroup: 2 (64 x 16 tiles, one wave per SIMD) or 4 (64 x 32, two).
// The values in the comments are those of WY_ = 2.
template <int WY_>
struct Shape {
    static_assert(WY_ == 2 || WY_ == 4, "64 x 16 or 64 x 32 tiles");
    static constexpr int WY = WY_;
    static constexpr int NW = WX * WY;                 // 4 waves
    static constexpr int NT = 64 * NW;                 // 256 threads
    static constexpr int TH = RB * WY;                 // 64 x 16 tile
    static constexpr int RTH = TH + 2 * HALO;          // 70 x 22 residual tile / patch
    static constexpr int PITCH = WY == 2 ? 28 : 44;    // bf16 elements per LDS column (>= RTH + 2; 56 / 88 B: 14 / 22 dwords between the
                                                       // columns of neighbouring lanes -- conflict-free b64 reads)
    static constexpr int COPY = RTC * PITCH;           // elements per shifted copy
    static constexpr int LDS_RT = 2 * 4 * COPY * 2;    // bytes: {hi,lo} x 4 row-shifted copies             (32256)
    static constexpr int SLAB = RTH * RTW;             // floats per col2im slab
    static constexpr int LDS_RSUM = 4 * SLAB * 4;      // 4 slabs by wave parity (wxi&1, wyi&1): waves sharing a slab
                                                       // never touch the same word, slabs are summed in a fixed order
    static constexpr int LDS_TACC = NW * 64 * 4;
    static constexpr int LDS_STAGE = LDS_RT + LDS_RSUM + LDS_W + LDS_TAU + LDS_TACC;
    static constexpr int LDS_DA_THIN = 2 * 4 * TCOPY * 2;      // reverse stage with dA_k: r_k as [hl][shift] copies   (26496)
    static constexpr int LDS_DA = LDS_DA_THIN + NW * 2 * 2 * IMG_ELEMS * 2;   // + [wave][channel tile][hl] transposition images
    // One wave per SIMD: every weight fragment of the launch lives in the wave's registers; two: read from LDS where used
    static constexpr bool WREG = WY == 2;
};

struct FusedParams {
    const float *r;          // (N,H,W) thin input of the analysis-like half (r_k, yp, q_{k+1} or g_xp)
    const float *zin;        // (N,M,H,W) or nullptr: z_k (forward) / du_{k+1} (backward)
    unsigned *map;           // support/sign bit planes of z_{k+1}, (N,4,H,W) words: written by the forward
                             // (nullable), read by the backward instead of the fat z_{k+1} (see k_support_map)
    float *zout;             // (N,M,H,W): z_{k+1} (forward) / du_k (backward)
    const float *tau;        // forward: (N,M) thresholds
    float *dtau;             // backward: (numWG, M) per-workgroup partial sums of -sign(z_{k+1}) * du_k
    const uint4 *frags;      // prepared weights, see k_prep
    float *patches;          // (N,tilesY,tilesX,RTH,RTW)
    float sgn;               // u = zin + sgn * acc
    int do_synth;            // 0: skip the synthesis-like half (last backward stage)
    CDL_DBG_FIELD(int dbg;)  // probe build only (CDL_FUSED_DEBUG): 1 no stores, 2 no synthesis, 32 no LDS adds, 64 no ST,
                             // 4 no analysis MFMAs, 8 no thin loads (both operands), 16 no fat loads, 128 no per-tile phase
                             // behind the row loop (patch write-out, staging stores), 256 no threshold partials (neither the
                             // per-element sums nor their per-tile transposition: dtau comes out 0); results are wrong
    int N, H, W, tilesX, tilesY;
    int rev;                 // walk the tiles from the last to the first (see "snake order" at the sweeps)
    const float *r2;         // reverse stage with DA: (N,H,W) thin operand of dA_k = alpha * du_k (x) im2col(r2) (r_k or yp)
    float *da_partial;       // (gridDim.x, 2, M, 64): per-workgroup partial of dA_k in operator slot 0 (k_wgrad_reduce's layout)
    int drop_zout;           // backward: zout is not written (the sweep's last stage: du_0 is consumed in registers only)
};
// What the noise-level map modes take on top (MODE_*_MAP).  The host fills one FusedMapParams per
// launch; a kernel of another mode is declared with the base and receives the base part: its argument block is what it was.
struct FusedMapParams : FusedParams {
    const float *cmap;      // (N,H,W): forward threshold tau[n,m] + cmap[n,y,x] * tslope[m]; reverse: weight of the second partial
    const float *tslope;     // (M): the slopes t[k,1,:]
    float *dtau_w;           // backward: (numTiles, M) partial sums of -cmap * sign(z_{k+1}) * du_k, rows as dtau's
    float *dcmap;            // backward, nullable: (N,H,W) dL/dcmap, = or += (dc_add) sum_m tslope[m] * (-sign(z_{k+1}) du_k)
    int dc_add;
};

// The map modes are the three base modes with this bit set: the same kernel, a threshold per code element.
// (ints, not an unnamed enum: MODE_MAP enters the kernels' mangled names through StageParams, and the host and device
//  passes number unnamed types differently -- the host then registers a kernel name the code object does not hold)
constexpr int MODE_MAP = 4, MODE_FWD_MAP = MODE_FWD | MODE_MAP, MODE_FIRST_MAP = MODE_FIRST | MODE_MAP, MODE_BWD_MAP = MODE_BWD | MODE_MAP;
template <int MODE_M> using StageParams = std::conditional_t<(MODE_M & MODE_MAP) != 0, FusedMapParams, FusedParams>;

// ------------------------------------------------------------------------------------------
// Weight preparation: fp32 filters -> bf16 hi/lo MFMA A-operand fragments.
//   analysis  frag f = R*4 + ks, lane (row = ch - 32R, h), element jj:  W_A[ch][i = jj][j = 2ks + h]
//             (k = 8*j + i, so that one lane's 8 k-values are 8 consecutive ROWS of the residual)
//   synthesis frag f = Rp*(2MT) + 2R + s, lane (row = tap - 32Rp, h), element jj:
//             W_B[ch = 32R + 16s + 8(jj>>2) + 4h + (jj&3)][tap], tap = 8*i + j -- the k order in which
//             a 32x32 accumulator tile presents itself as the next MFMA's B operand.
// Output: [A hi | A lo | B hi | B lo], each frag = 64 lanes x 16 B.
__device__ __forceinline__ float embed7(const float *w, int P, int i, int j)
{
    const int off = (7 - P) / 2;
    const int ii = i - off, jj = j - off;
    if (i > 6 || j > 6 || ii < 0 || jj < 0 || ii >= P || jj >= P) return 0.0f;
    return w[ii * P + jj];
}

__device__ __forceinline__ void prep_one(const float *__restrict__ wA, const float *__restrict__ wB,
                                         uint4 *__restrict__ out, int MT, int P, int t)
{
    const int FA = MT * 4, FB = 4 * MT;
    if (t >= (FA + FB) * 64) return;
    const int lane = t & 63, f = t >> 6;
    const int row = lane & 31, h = lane >> 5;
    const int PP = P * P;
    float v[8];
    if (f < FA) {
        const int R = f / 4, ks = f % 4;
        const int ch = 32 * R + row;
#pragma unroll
        for (int jj = 0; jj < 8; ++jj) v[jj] = embed7(wA + (size_t)ch * PP, P, jj, 2 * ks + h);
    } else {
        const int g = f - FA;
        const int Rp = g / (2 * MT), ksB = g % (2 * MT);
        const int R = ksB >> 1, s = ksB & 1;
        const int tap = 32 * Rp + row;
#pragma unroll
        for (int jj = 0; jj < 8; ++jj) {
            const int ch = 32 * R + 16 * s + 8 * (jj >> 2) + 4 * h + (jj & 3);
            v[jj] = embed7(wB + (size_t)ch * PP, P, tap >> 3, tap & 7);
        }
    }
    bf16x8 hi, lo;
#pragma unroll
    for (int jj = 0; jj < 8; ++jj) {
        __bf16 hh, ll;
        split_bf16(v[jj], hh, ll);
        hi[jj] = hh;
        lo[jj] = ll;
    }
    uint4 *hi_dst, *lo_dst;
    if (f < FA) { hi_dst = out + (size_t)f * 64; lo_dst = out + (size_t)(FA + f) * 64; }
    else { hi_dst = out + (size_t)(2 * FA + (f - FA)) * 64; lo_dst = out + (size_t)(2 * FA + FB + (f - FA)) * 64; }
    hi_dst[lane] = __builtin_bit_cast(uint4, hi);
    lo_dst[lane] = __builtin_bit_cast(uint4, lo);
}

__global__ void k_prep(const float *__restrict__ wA, const float *__restrict__ wB,
                       uint4 *__restrict__ out, int MT, int P)
{
    prep_one(wA, wB, out, MT, P, blockIdx.x * blockDim.x + threadIdx.x);
}

// every (A, B) pair of a sweep in one launch: pair = blockIdx.y, its fragments at out + pair * frag_uint4
constexpr int PREP_BATCH = 32;
struct PrepBatch {
    const float *wA[PREP_BATCH];
    const float *wB[PREP_BATCH];
};
__global__ void k_prep_batch(PrepBatch b, uint4 *__restrict__ out, int frag_uint4, int MT, int P)
{
    prep_one(b.wA[blockIdx.y], b.wB[blockIdx.y], out + (size_t)blockIdx.y * frag_uint4, MT, P,
             blockIdx.x * blockDim.x + threadIdx.x);
}

// Fat tensors are addressed through buffer descriptors: the descriptor covers one image's (M,H,W)
// block, the per-lane part of the address is ONE 32-bit VGPR byte offset shared by every channel of
// the block and the channel stride goes in an SGPR -- no 64-bit per-access address registers, and an
// out-of-image lane simply carries an out-of-range offset (loads return 0, stores are dropped).
// Cache policy per stream: the aux immediate of the buffer builtins (0 plain; 1 sc0; 2 nt, streaming; 16 sc1 -- a store
// writes through the XCD's L2, a load goes past the CU's L1; 17 sc0 sc1; 18 nt sc1).  A policy changes where a line is
// kept, never a value.  One constant per stream, each the winner of tools/probes/probe_stream.hip "policy" and of an A/B of
// the training step against the parent; the -D overrides are for A/B builds.  A fat tensor is read
// once per launch and is 34 times the L2s' size: its loads stream (nt) -- the read-only k_wgrad2d gains 16 %, the stages
// 3 %; no store policy measured a gain.  Streams that are not named here go through plain pointers and keep the default
// policy (the support map, patches, partial banks, k_assemble: the dependent boundary behind 30 MB of 16-byte stores
// costs 17 us under every policy, and a write-through patch store moved nothing).
#ifndef CDL_POL_STAGE_FAT_LD
#define CDL_POL_STAGE_FAT_LD 2
#endif
#ifndef CDL_POL_STAGE_FAT_ST
#define CDL_POL_STAGE_FAT_ST 0
#endif
#ifndef CDL_POL_WGRAD_FAT_LD
#define CDL_POL_WGRAD_FAT_LD 2
#endif
// The reverse stage's row loop, each piece with a -D override for A/B builds like the policies above:
// the threshold partials written into the synthesis k-steps, their per-tile transposition by DPP instead of through LDS, and
// the next row block's fat inputs issued behind the epilogue of this one.  None of them changes a value.
#ifndef CDL_STAGE_TSUM_SHADOW
#define CDL_STAGE_TSUM_SHADOW 1
#endif
#ifndef CDL_STAGE_TSUM_DPP
#define CDL_STAGE_TSUM_DPP 1
#endif
#ifndef CDL_STAGE_PREFETCH
#define CDL_STAGE_PREFETCH 1
#endif
struct CachePolicy {
    static constexpr int stage_fat_ld = CDL_POL_STAGE_FAT_LD;   // k_stage: z_k / du_{k+1}, 16 B per lane (LAY_BLK)
    static constexpr int stage_fat_st = CDL_POL_STAGE_FAT_ST;   // k_stage: z_{k+1} / du_k, 16 B per lane (LAY_BLK)
    static constexpr int wgrad_fat_ld = CDL_POL_WGRAD_FAT_LD;   // k_wgrad2d: z_{k-1} / du_k, 16 B per lane (LAY_BLK)
    // accesses narrower than 16 B -- NCHW dwords, bf16 storage (LAY_BLK16) -- in every kernel: never measured with a
    // policy, and a write-through store of 4 or 8 bytes is a fabric write of its own
    static constexpr int narrow = 0;
};
__device__ __forceinline__ __amdgpu_buffer_rsrc_t fat_rsrc(const float *base, size_t img_floats)
{
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(base), 0, (int)(img_floats * 4), 0x00020000);
}
__device__ __forceinline__ float buf_ld(__amdgpu_buffer_rsrc_t r, int voff, int soff)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, voff, soff, CachePolicy::narrow));
}
__device__ __forceinline__ void buf_st(float v, __amdgpu_buffer_rsrc_t r, int voff, int soff)
{
    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), r, voff, soff, CachePolicy::narrow);
}

// ---- layouts of the fat tensors ------------------------------------------------------------------------
// LAY_NCHW : the reference's (N, M, H, W) fp32.  A wave instruction of the MFMA C/D layout (lane = pixel,
//            register = channel) touches two 128-B segments in two channel planes; 32 dword accesses per
//            32-pixel row block.  What callers see (z_K, user gradients) is always this.
// LAY_BLK  : pixel-blocked fp32 [n][y][x/32][M/4][32 px][4 ch] for tensors that stay INSIDE a sweep (z_1 ..
//            z_{K-1}, du_k): the 4 consecutive channels a lane owns per register quad are 16 contiguous
//            bytes, a wave instruction covers 1 KiB contiguous, a row block 8 KiB contiguous -- 8 dwordx4
//            accesses, no shuffles.  tools/probes/probe_stream.hip (same box, pure load -> store stream of
//            the cfg2 code tensor): plane-strided dwords 5.08 TB/s, this 5.65 TB/s.
// LAY_BLK16: the same blocking with bf16 elements (8 bytes per lane): opt-in reduced-precision STORAGE
//            (half the fat bytes; the 1e-5 parity gate does not hold in this mode).
enum { LAY_NCHW = 0, LAY_BLK = 1, LAY_BLK16 = 2 };
typedef __attribute__((ext_vector_type(2))) unsigned u32x2;

__host__ __device__ inline size_t blk_image_elems(int M, int H, int W) { return (size_t)H * ((W + 31) / 32) * M * 32; }
template <int LAY> __host__ __device__ inline size_t lay_image_bytes(int M, int H, int W)
{
    return LAY == LAY_NCHW ? (size_t)M * H * W * 4 : blk_image_elems(M, H, W) * (LAY == LAY_BLK ? 4 : 2);
}

// (buffer descriptors from wave-uniform pointers: uniform_rsrc, cdl_wave_dev.h)

// round-to-nearest-even fp32 -> bf16 -> fp32 (what a bf16-stored code tensor holds)
__device__ __forceinline__ float bf16_round(float v) { return (float)(__bf16)v; }

// 16 consecutive-quad accesses of one accumulator tile set: registers 4q..4q+3 of tile R are channels
// 32R + 8q + 4h + (0..3) = quad 8R + 2q + h of the blocked layout; `voff` carries (y, xb, h, c), the
// scalar offset the quad pair.
// LAY_BLK16 loads kept PACKED (two bf16 per register): decoded where the values are consumed, so that the wait for
// the loads lands there and not right behind their issue (decoding at the load serialised load latency and the
// GEMM that should cover it: 0.62 against 0.44 ms for the fp32 layout)
template <int MT>
__device__ __forceinline__ void blk16_load_raw(u32x2 (&z)[MT][4], __amdgpu_buffer_rsrc_t rs, int voff)
{
#pragma unroll
    for (int R = 0; R < MT; ++R)
#pragma unroll
        for (int q = 0; q < 4; ++q)
            z[R][q] = __builtin_bit_cast(u32x2, __builtin_amdgcn_raw_buffer_load_b64(rs, voff, (8 * R + 2 * q) * 32 * 8, CachePolicy::narrow));
}
__device__ __forceinline__ float blk16_decode(const u32x2 &u, int e)
{
    const unsigned w = (e & 2) ? u.y : u.x;
    return __builtin_bit_cast(float, (e & 1) ? (w & 0xffff0000u) : (w << 16));
}

// POL: the stream's CachePolicy constant (16-byte accesses only)
template <int LAY, int MT, int POL>
__device__ __forceinline__ void blk_load(float (&z)[MT][16], __amdgpu_buffer_rsrc_t rs, int voff)
{
    constexpr int EB = LAY == LAY_BLK ? 16 : 8;
#pragma unroll
    for (int R = 0; R < MT; ++R)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int soff = (8 * R + 2 * q) * 32 * EB;
            if constexpr (LAY == LAY_BLK) {
                typedef __attribute__((ext_vector_type(4))) float f32x4;
                const f32x4 f = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, voff, soff, POL));
                z[R][4 * q + 0] = f.x; z[R][4 * q + 1] = f.y; z[R][4 * q + 2] = f.z; z[R][4 * q + 3] = f.w;
            } else {
                const u32x2 u = __builtin_bit_cast(u32x2, __builtin_amdgcn_raw_buffer_load_b64(rs, voff, soff, CachePolicy::narrow));
                z[R][4 * q + 0] = __builtin_bit_cast(float, u.x << 16);
                z[R][4 * q + 1] = __builtin_bit_cast(float, u.x & 0xffff0000u);
                z[R][4 * q + 2] = __builtin_bit_cast(float, u.y << 16);
                z[R][4 * q + 3] = __builtin_bit_cast(float, u.y & 0xffff0000u);
            }
        }
}
// (values of a LAY_BLK16 store must already be bf16-representable: the caller rounds, so that the value it goes
//  on computing with is the stored one)
template <int LAY, int POL>
__device__ __forceinline__ void blk_store4(float a0, float a1, float a2, float a3, __amdgpu_buffer_rsrc_t rs, int voff, int quad_pair)
{
    constexpr int EB = LAY == LAY_BLK ? 16 : 8;
    const int soff = quad_pair * 32 * EB;
    if constexpr (LAY == LAY_BLK) {
        // The quad's constant offset goes into the VECTOR offset (the compiler folds it into the instruction's immediate
        // field, or one add), the scalar offset stays the literal 0.  A store of more than 64 bits reads its data registers
        // late: a vector instruction that writes one of them needs a wait state behind the store.  The compiler's hazard
        // recogniser pads that only when the store has no scalar-offset REGISTER; with the offset in an SGPR it let the
        // reverse stage <M = 64, plain bf16, blocked -> blocked, no dA_k> refill a staging quad in the instruction after
        // the store that read it, and du_k arrived with another quad's values, differently from call to call (DESIGN.md
        // sections 6b and 30).  (voff = OOB plus these offsets stays beyond every descriptor.)
        // Any further store of more than 8 bytes through a buffer descriptor must likewise keep its scalar offset an immediate.
        typedef __attribute__((ext_vector_type(4))) float f32x4;
        const f32x4 f = {a0, a1, a2, a3};
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, f), rs, voff + soff, 0, POL);
    } else {
        u32x2 u;
        u.x = (__builtin_bit_cast(unsigned, a0) >> 16) | (__builtin_bit_cast(unsigned, a1) & 0xffff0000u);
        u.y = (__builtin_bit_cast(unsigned, a2) >> 16) | (__builtin_bit_cast(unsigned, a3) & 0xffff0000u);
        __builtin_amdgcn_raw_buffer_store_b64(u, rs, voff, soff, CachePolicy::narrow);
    }
}

// a or b by a compile-time flag, where the two have different types
template <bool FIRST, class A, class B>
__device__ __forceinline__ decltype(auto) pick_ref(A &a, B &b)
{
    if constexpr (FIRST) return (a);
    else return (b);
}

// LaneTransposeSum (cdl_wave_dev.h; the DPP form: called once per tile by every lane of every wave) with the two halves of
// each of 16 totals joined
template <int N>
__device__ __forceinline__ float lane_transpose_sum(const float (&v)[N], int c)
{
    float r = LaneTransposeSum<N, CDL_STAGE_TSUM_DPP != 0>::run(v, c);
    if (N == 16) r += __shfl_xor(r, 16, 64);           // lanes c and c^16 hold halves of the same index
    return r;
}

// col2im, column direction, for one halo row: lane (c, h) holds tap columns j = 4h + (0..3) of pixel
// column c; returns on lane L (0..37) the sum over j of the value of column L - j.  The upper half's
// taps are first moved onto the lower lanes, then a 6-step Horner chain of DPP wave shifts lets the
// terms that leave column 31 collect on lanes 32..37 (the overlap with the next wave's columns).
__device__ __forceinline__ float col2im_row(const float (&rv)[4], int h)
{
    const float r4 = upper_half_to_lower(rv[0]);
    const float r5 = upper_half_to_lower(rv[1]);
    const float r6 = upper_half_to_lower(rv[2]);
    const bool lo = h == 0;
    float s = lo ? r6 : 0.0f;
    s = wave_shr1(s) + (lo ? r5 : 0.0f);
    s = wave_shr1(s) + (lo ? r4 : 0.0f);
    s = wave_shr1(s) + (lo ? rv[3] : 0.0f);
    s = wave_shr1(s) + (lo ? rv[2] : 0.0f);
    s = wave_shr1(s) + (lo ? rv[1] : 0.0f);
    s = wave_shr1(s) + (lo ? rv[0] : 0.0f);
    return s;
}

// Thin-tile staging: a thread stages a RUN of 8 elements along the contiguous axis of the shifted LDS copies (rows of one
// column for the row-shifted copies of the stage's thin input, columns of one row for the column-shifted copies of dA_k's).
// store_run<S> writes one run into the copy shifted by S (0..3): element j lands on dst[j - S]; dst is 8-byte aligned, so
// the stores are as wide as the shift allows -- 2 + 4 + 3 + 4 = 13 for the four copies of a run where one element at a
// time took 32.  low: the run starts at the copy's edge and the S elements that would land in front of it are dropped.
constexpr int RUN = 8;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
template <int S>
__device__ __forceinline__ void store_run(__bf16 *dst, const __bf16 (&v)[RUN], bool low)
{
    static_assert(S >= 0 && S <= 3, "four shifted copies");
    if (!low) {
        if constexpr (S == 1) dst[-1] = v[0];
        if constexpr (S == 2) *reinterpret_cast<bf16x2 *>(dst - 2) = bf16x2{v[0], v[1]};
        if constexpr (S == 3) { dst[-3] = v[0]; *reinterpret_cast<bf16x2 *>(dst - 2) = bf16x2{v[1], v[2]}; }
    }
    *reinterpret_cast<bf16x4 *>(dst) = bf16x4{v[S], v[S + 1], v[S + 2], v[S + 3]};
    if constexpr (S == 0) *reinterpret_cast<bf16x4 *>(dst + 4) = bf16x4{v[4], v[5], v[6], v[7]};
    if constexpr (S == 1) { *reinterpret_cast<bf16x2 *>(dst + 4) = bf16x2{v[5], v[6]}; dst[6] = v[7]; }
    if constexpr (S == 2) *reinterpret_cast<bf16x2 *>(dst + 4) = bf16x2{v[6], v[7]};
    if constexpr (S == 3) dst[4] = v[7];
}
// the hi / lo split of a run and its four shifted copies: copy S of half hl at dst + (4 * hl + S) * copy_elems
template <int PREC>
__device__ __forceinline__ void store_run_copies(__bf16 *dst, int copy_elems, const float (&f)[RUN], bool low)
{
    __bf16 hh[RUN], ll[RUN];
#pragma unroll
    for (int j = 0; j < RUN; ++j) split_bf16(f[j], hh[j], ll[j]);
    store_run<0>(dst, hh, low); store_run<1>(dst + copy_elems, hh, low);
    store_run<2>(dst + 2 * copy_elems, hh, low); store_run<3>(dst + 3 * copy_elems, hh, low);
    if (PREC != 1) {
        dst += 4 * copy_elems;
        store_run<0>(dst, ll, low); store_run<1>(dst + copy_elems, ll, low);
        store_run<2>(dst + 2 * copy_elems, ll, low); store_run<3>(dst + 3 * copy_elems, ll, low);
    }
}

// ------------------------------------------------------------------------------------------
// Phases k_stage and k_wgrad2d share, one copy each.  Plain functions with the accumulator arrays
// passed by reference, not closures: cdl_strip_dev.h records what a closure around an accumulator set cost.  dA_k from
// the stage's ride and from k_wgrad2d are compared bit for bit: both call the SAME product sequence below.

// tile t of a launch's walk (from the last tile to the first with rev): its index, image and tile row / column.  t may
// lie past the last tile (a load a tile ahead): the caller then uses none of the fields.
struct TileAt { int tile, n, tyi, txi; };
__device__ __forceinline__ TileAt tile_decode(int t, int numTiles, int tilesX, int tilesY, int rev)
{
    TileAt q;
    q.tile = rev ? numTiles - 1 - t : t;
    int bid = q.tile;
    q.txi = bid % tilesX; bid /= tilesX;
    q.tyi = bid % tilesY;
    q.n = bid / tilesY;
    return q;
}

// eight consecutive bf16 from an 8-byte aligned LDS element (two b64 reads: the shifted copies guarantee no more)
__device__ __forceinline__ bf16x8 lds_window8(const __bf16 *p)
{
    const bf16x4 a0 = *reinterpret_cast<const bf16x4 *>(p);
    const bf16x4 a1 = *reinterpret_cast<const bf16x4 *>(p + 4);
    return __builtin_shufflevector(a0, a1, 0, 1, 2, 3, 4, 5, 6, 7);
}

template <int N>
__device__ __forceinline__ void zero_tiles(f32x16 (&a)[N])
{
#pragma unroll
    for (int i = 0; i < N; ++i)
#pragma unroll
        for (int v = 0; v < 16; ++v) a[i][v] = 0.0f;
}

// Per-channel values of an LDS [64] array in accumulator-register order: register v of tile R on a lane of half h is
// channel 32R + 8(v>>2) + 4h + (v&3).  One float4 quad (registers 4qv .. 4qv + 3), or all of the lane's 16 MT values.
__device__ __forceinline__ float4 lane_channel_quad(const float *src, int R, int qv, int h)
{
    return *reinterpret_cast<const float4 *>(&src[32 * R + 8 * qv + 4 * h]);
}
template <int MT>
__device__ __forceinline__ void lane_channel_values(float (&out)[MT * 16], const float *src, int h)
{
#pragma unroll
    for (int R = 0; R < MT; ++R)
#pragma unroll
        for (int qv = 0; qv < 4; ++qv) {
            const float4 s4 = lane_channel_quad(src, R, qv, h);
            out[16 * R + 4 * qv + 0] = s4.x; out[16 * R + 4 * qv + 1] = s4.y;
            out[16 * R + 4 * qv + 2] = s4.z; out[16 * R + 4 * qv + 3] = s4.w;
        }
}

// Filter gradient, step 1: one channel quad of a row block -- channels 8qv + 4h .. + 3 of a 32-channel tile at pixel
// column c -- into the tile's [pixel][32 ch] transposition image (64-B rows, 8-byte slots XOR-swizzled by (pixel>>1)&7:
// conflict-free stores); the lo image follows the hi image.  ALO: the fat operand has a lo part.
template <bool ALO>
__device__ __forceinline__ void wgrad_transpose_store(__bf16 *img, int qv, int c, int h, bf16x4 hi4, bf16x4 lo4)
{
    const int slot = (2 * qv + h) ^ ((c >> 1) & 7);      // 8-byte slot of channels 8qv+4h..+3
    __bf16 *dst = img + c * 32 + slot * 4;
    *reinterpret_cast<bf16x4 *>(dst) = hi4;
    if (ALO) *reinterpret_cast<bf16x4 *>(dst + IMG_ELEMS) = lo4;
}
template <bool ALO>
__device__ __forceinline__ void wgrad_transpose_store(__bf16 *img, int qv, int c, int h, float v0, float v1, float v2, float v3)
{
    const float val[4] = {v0, v1, v2, v3};
    bf16x4 hi4, lo4;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        __bf16 hh, ll;
        split_bf16(val[e], hh, ll);
        hi4[e] = hh;
        lo4[e] = ll;
    }
    wgrad_transpose_store<ALO>(img, qv, c, h, hi4, lo4);
}

// Filter gradient, step 2: acc[R][tt] += X[32 ch of tile R][32 px] * im2col(T)[32 px][32 taps of tile tt] for one row
// block of a wave, behind the wave barrier that follows the stores above.  wimg: the wave's [R][hl] images; thin_hi: the
// four column-shifted hi copies of the thin tile ([s][TCOPY], the lo copies 4 * TCOPY behind); yl: tile-local image row.
// The order of the products per (R, tt) -- lo*hi, hi*lo, [lo*lo], hi*hi -- is part of the result's bits.  Every lane of
// the wave must be active (the transposed reads gather across lanes).
template <int MT, int PREC, bool ALO>
__device__ __forceinline__ void wgrad_products(f32x16 (&acc)[MT][2], const __bf16 *wimg, const __bf16 *thin_hi, int yl,
                                               int wxi, int lane)
{
    const int c = lane & 31, h = lane >> 5;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
        // B fragments: tap column of this lane, 8 consecutive pixels 16kk + 8h + (0..7)
        bf16x8 Bh[2], Bl[2];
#pragma unroll
        for (int tt = 0; tt < 2; ++tt) {
            const int tap = 32 * tt + c, ti = tap >> 3, tj = tap & 7;
            const int e0 = wxi * 32 + 16 * kk + 8 * h + (tj & 4);
            const __bf16 *ph = thin_hi + (tj & 3) * TCOPY + (yl + ti) * TPITCH + e0;
            Bh[tt] = lds_window8(ph);
            if (PREC != 1) Bl[tt] = lds_window8(ph + 4 * TCOPY);
        }
#pragma unroll
        for (int R = 0; R < MT; ++R) {
            // A fragments by transposed reads: lane (i = lane&15 of group g) gets channel
            // 16(g&1) + i, pixels 16kk + 8h + 4*half + (0..3)
            const int gg = (lane >> 4) & 1, qq = (lane >> 2) & 3, pp = lane & 3;
            bf16x4 part[2][2];
#pragma unroll
            for (int half = 0; half < 2; ++half) {
                const int row = 16 * kk + 8 * h + 4 * half + qq;
                const int slot = (4 * gg + pp) ^ ((row >> 1) & 7);
                const __bf16 *src = wimg + (size_t)(R * 2) * IMG_ELEMS + row * 32 + slot * 4;
                part[0][half] = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
                    (__attribute__((address_space(3))) bf16x4 *)(src));
                if (ALO)
                    part[1][half] = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
                        (__attribute__((address_space(3))) bf16x4 *)(src + IMG_ELEMS));
            }
            const bf16x8 Ah = __builtin_shufflevector(part[0][0], part[0][1], 0, 1, 2, 3, 4, 5, 6, 7);
            bf16x8 Al;
            if (ALO) Al = __builtin_shufflevector(part[1][0], part[1][1], 0, 1, 2, 3, 4, 5, 6, 7);
#pragma unroll
            for (int tt = 0; tt < 2; ++tt) {
                if (PREC != 1) {
                    if (ALO) acc[R][tt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(Al, Bh[tt], acc[R][tt], 0, 0, 0);
                    acc[R][tt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(Ah, Bl[tt], acc[R][tt], 0, 0, 0);
                    if (PREC == 2 && ALO) acc[R][tt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(Al, Bl[tt], acc[R][tt], 0, 0, 0);
                }
                acc[R][tt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(Ah, Bh[tt], acc[R][tt], 0, 0, 0);
            }
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// Filter gradient, step 3: the NWS waves of a sum add their [ch][tap] accumulators through LDS -- wave 0 stores, the
// others add in turn: a fixed order, every lane owns its words -- into operator slot `slot` of red ([NSLOT][M][64]),
// and the workgroup (64 * NWS * NSLOT threads, all of which call this) copies red out as its partial, in
// k_wgrad_reduce's layout.  w: this wave's place in its sum.
template <int MT, int NWS, int NSLOT>
__device__ __forceinline__ void wgrad_wave_sum(const f32x16 (&acc)[MT][2], float *red, int slot, int w_mine, int tid,
                                               float *dst)
{
    constexpr int M = 32 * MT;
    const int c = tid & 31, h = (tid >> 5) & 1;
    for (int w = 0; w < NWS; ++w) {
        __syncthreads();
        if (w_mine == w) {
#pragma unroll
            for (int R = 0; R < MT; ++R)
#pragma unroll
                for (int tt = 0; tt < 2; ++tt)
#pragma unroll
                    for (int v = 0; v < 16; ++v) {
                        const int ch = 32 * R + (v & 3) + 8 * (v >> 2) + 4 * h;
                        float *dstw = &red[(slot * M + ch) * 64 + 32 * tt + c];
                        *dstw = (w == 0 ? 0.0f : *dstw) + acc[R][tt][v];
                    }
        }
    }
    __syncthreads();
    for (int i = tid; i < NSLOT * M * 64; i += 64 * NWS * NSLOT) dst[i] = red[i];
}

// reverse stage: the wave's sum of each per-lane threshold partial, into the wave's [64] row of an LDS [wave][64] array.
// lane c of each half holds the wave's sum for accumulator index i = c mod (16 MT):
// register v = i & 15 of tile R = i >> 4  ->  channel 32R + 8(v>>2) + 4h + (v&3)
template <int MT>
__device__ __forceinline__ void tsum_to_lds(const float (&tsum)[MT * 16], float *tacc_wave, int c, int h)
{
    const float tacc = lane_transpose_sum(tsum, c);
    if (c < MT * 16) {
        const int R = c >> 4, v = c & 15;
        tacc_wave[32 * R + 8 * (v >> 2) + 4 * h + (v & 3)] = tacc;
    }
}

// ------------------------------------------------------------------------------------------
// MODE_FWD / MODE_FIRST: zout = ST(zin + sgn * A r, tau)              (net.py:85,87)
// MODE_BWD            : zout = [z_{k+1} != 0] * (zin + A-like r),  dtau partials   (reverse sweep);
//                       support and sign of z_{k+1} come from the 2-bit map, not from the fat tensor
//   LIN / LOUT: layouts of zin and zout (LAY_*)
//   DA (reverse stage only): the filter gradient dA_k = du_k (x) im2col(r2) rides in the launch -- du_k is transposed per row
//   block through wave-private LDS images exactly as k_wgrad2d does it, and accumulated in 2 x MT more accumulator tiles
//   WY: the tile shape (Shape<WY>)
//   MODE_M | MODE_MAP: a noise-level map.  Forward: p.tau holds t[k,0,:] (for every sample), the slopes
//   t[k,1,:] sit in the lane's registers beside them and each lane loads cm = cmap[n,y,x] once per row block: the threshold of
//   channel m at its pixel is cdl_map_threshold(t0[m], cm, t1[m]), the reference's bit for bit.  Reverse: a second, map-weighted
//   set of threshold partials (p.dtau_w) and, with p.dcmap, dL/dcmap = sum_m t1[m] g[m] over the lane's channels and its
//   partner half's.  Everything map-specific is behind `if constexpr (MAP)`: the other modes compile to what they were.
template <int MT, int PREC, int MODE_M, int LIN, int LOUT, bool DA = false, int WY = 2>
__global__ __launch_bounds__(Shape<WY>::NT) void k_stage(StageParams<MODE_M> p)
{
    constexpr int MODE = MODE_M & ~MODE_MAP;
    constexpr bool MAP = (MODE_M & MODE_MAP) != 0;
    using G = Shape<WY>;
    constexpr int NW = G::NW, NT = G::NT, TH = G::TH, RTH = G::RTH, PITCH = G::PITCH, COPY = G::COPY, SLAB = G::SLAB;
    constexpr int LDS_RT = G::LDS_RT, LDS_RSUM = G::LDS_RSUM, LDS_STAGE = G::LDS_STAGE, LDS_DA_THIN = G::LDS_DA_THIN;
    static_assert(!DA || (MODE == MODE_BWD && TH == GW_TH), "dA_k rides in the reverse stage, on k_wgrad2d's 64 x 16 tiles");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __bf16 *rt = reinterpret_cast<__bf16 *>(smem);                               // [hl][q][col][PITCH]
    float *rsum_all = reinterpret_cast<float *>(smem + LDS_RT);                   // [4][RTH][RTW]
    const uint4 *wl = reinterpret_cast<const uint4 *>(smem + LDS_RT + LDS_RSUM);  // weight fragments
    float *tau_s = reinterpret_cast<float *>(smem + LDS_RT + LDS_RSUM + LDS_W);
    float *tacc_s = tau_s + 64;                                                   // backward: [wave][64]
    __bf16 *thin2 = reinterpret_cast<__bf16 *>(smem + LDS_STAGE);                 // DA: [hl][s][TCOPY] copies of r2's tile
    __bf16 *imgs2 = reinterpret_cast<__bf16 *>(smem + LDS_STAGE + LDS_DA_THIN);   // DA: [wave][R][hl][IMG_ELEMS]
    // MAP: the slopes live where the mode has no use for the area -- forward: tacc_s[0..M), reverse: tau_s; the reverse's
    // weighted [wave][64] sums behind everything else (stage_lds_bytes)
    float *slope_s = MODE == MODE_BWD ? tau_s : tacc_s;
    float *tacc_w_s = reinterpret_cast<float *>(smem + LDS_STAGE + (DA ? G::LDS_DA : 0));

    constexpr int M = 32 * MT;
    constexpr int FA = MT * 4, FB = 4 * MT;
    constexpr int NFRAG = (PREC != 1 ? 2 : 1) * (FA + FB);   // bf16 mode stages only the hi fragments
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wxi = wid % WX, wyi = wid / WX;
    const int c = lane & 31, h = lane >> 5;
    const size_t HW = (size_t)p.H * p.W;
    const int numTiles = p.N * p.tilesY * p.tilesX;

    // ---- once per workgroup: zero LDS, weight fragments -> LDS
    {
        uint4 *z4 = reinterpret_cast<uint4 *>(smem);
        for (int i = tid; i < (LDS_RT + LDS_RSUM) / 16; i += NT) z4[i] = make_uint4(0, 0, 0, 0);
        uint4 *wdst = reinterpret_cast<uint4 *>(smem + LDS_RT + LDS_RSUM);
        if (PREC != 1) {
            for (int i = tid; i < NFRAG * 64; i += NT) wdst[i] = p.frags[i];
        } else {                                            // [A hi | B hi] compacted
            for (int i = tid; i < FA * 64; i += NT) wdst[i] = p.frags[i];
            for (int i = tid; i < FB * 64; i += NT) wdst[FA * 64 + i] = p.frags[2 * FA * 64 + i];
        }
        if constexpr (MAP) {
            if (tid < M) slope_s[tid] = p.tslope[tid];       // one launch, one iteration: the slopes never change
        }
    }
    // thin-tile staging: registers first (so the next tile's loads fly during this tile's GEMMs), then
    // 4 row-shifted bf16 hi/lo copies in LDS.  Every in-tile word is rewritten per tile (zeros outside
    // the image); the pad words stay zero from the pass above.  A thread owns the same run of every tile -- RUN rows of
    // one column (store_run) -- so what depends on (tid) alone is computed here, once: only the tile origin changes.
    // Rows RTH.. of a column's last run are staged as zeros: they land on pad words.
    constexpr int RT_RUNS = (RTH + RUN - 1) / RUN;           // runs per column (3)
    static_assert(RTW * RT_RUNS <= NT && RT_RUNS * RUN <= PITCH, "one run per thread; a column's runs stay inside its pitch");
    const int rt_xx = tid % RTW, rt_y0 = (tid / RTW) * RUN;
    const bool rt_on = tid < RTW * RT_RUNS;
    __bf16 *const rt_dst = rt + rt_xx * PITCH + rt_y0;
    float stg[RUN];
    auto stage_load = [&](int t) {
        const TileAt q = tile_decode(t, numTiles, p.tilesX, p.tilesY, p.rev);
        const float *rimg = p.r + (size_t)q.n * HW;
        const int gy0 = q.tyi * TH - HALO + rt_y0, gx = q.txi * TW - HALO + rt_xx;
        const bool colok = rt_on && t < numTiles && !CDL_DBG(p.dbg, 8) && gx >= 0 && gx < p.W;
#pragma unroll
        for (int j = 0; j < RUN; ++j) {
            const int gy = gy0 + j;
            float v = 0.0f;
            if (colok && rt_y0 + j < RTH && gy >= 0 && gy < p.H) v = rimg[(size_t)gy * p.W + gx];
            stg[j] = v;
        }
    };
    auto stage_store = [&]() {
        if (rt_on) store_run_copies<PREC>(rt_dst, COPY, stg, rt_y0 == 0);
    };
    // DA: the tile of r2 under this tile (22 x 70 with the halo), as 4 column-shifted bf16 hi/lo copies (k_wgrad2d's
    // format: every 8-pixel window of an im2col row 8-byte aligned); loaded a tile ahead like the thin input: into
    // registers in front of the row loop, into LDS behind the barrier that ends it.  A run is RUN columns of one row;
    // columns RTW.. of a row's last run are staged as zeros (pad words)
    constexpr int T2_RUNS = (RTW + RUN - 1) / RUN;           // runs per row (9)
    static_assert(!DA || (GW_RTH * T2_RUNS <= NT && T2_RUNS * RUN <= TPITCH), "one run per thread; a row's runs stay inside its pitch");
    const int t2_x0 = (tid % T2_RUNS) * RUN, t2_yy = tid / T2_RUNS;
    const bool t2_on = tid < GW_RTH * T2_RUNS;
    __bf16 *const t2_dst = thin2 + t2_yy * TPITCH + t2_x0;
    float stg2[DA ? RUN : 1];
    auto stage2_load = [&](int t) {
        const TileAt q = tile_decode(t, numTiles, p.tilesX, p.tilesY, p.rev);
        const float *timg = p.r2 + (t < numTiles ? (size_t)q.n * HW : 0);    // (past the last tile: nothing is read)
        const int gy = q.tyi * TH - HALO + t2_yy, gx0 = q.txi * TW - HALO + t2_x0;
        const bool rowok = t2_on && t < numTiles && !CDL_DBG(p.dbg, 8) && gy >= 0 && gy < p.H;
#pragma unroll
        for (int j = 0; j < (DA ? RUN : 1); ++j) {
            const int gx = gx0 + j;
            const bool ok = rowok && t2_x0 + j < RTW && gx >= 0 && gx < p.W;
            const float v = timg[ok ? (size_t)gy * p.W + gx : 0];
            stg2[j] = ok ? v : 0.0f;
        }
    };
    auto stage2_store = [&]() {
        if constexpr (DA) {
            if (t2_on) store_run_copies<PREC>(t2_dst, TCOPY, stg2, t2_x0 == 0);
        }
    };
    f32x16 dacc[DA ? MT : 1][2];              // DA: dA_k[channel tile][tap tile], over every tile of this workgroup
    if constexpr (DA) {
#pragma unroll
        for (int R = 0; R < MT; ++R) zero_tiles(dacc[R]);
        // pad elements of the copies are read (into ignored tap columns) and must stay finite
        for (int i = tid; i < LDS_DA_THIN / 16; i += NT) reinterpret_cast<uint4 *>(thin2)[i] = make_uint4(0, 0, 0, 0);
        stage2_load(blockIdx.x);
    }
    stage_load(blockIdx.x);
    __syncthreads();                                        // zero pass done before the first fill
    stage_store();
    if constexpr (DA) stage2_store();

    // fragment offsets inside the LDS weight area
    constexpr int OFF_AH = 0;
    constexpr int OFF_AL = FA;                               // split3 only
    constexpr int OFF_BH = (PREC != 1 ? 2 * FA : FA);
    constexpr int OFF_BL = 2 * FA + FB;                      // split3 only
    // One wave per SIMD: every weight fragment of the launch lives in this wave's registers (32 x 4 at M = 64, split3; the
    // 512-register budget has the room) -- with no partner wave on the SIMD, the LDS latency of a fragment read in front of
    // (almost) every MFMA was most of the row block's time.  Two waves per SIMD: read from LDS where used.
    constexpr bool WREG = G::WREG;
    bf16x8 wreg[WREG ? NFRAG : 1];
    if constexpr (WREG) {
#pragma unroll
        for (int f = 0; f < NFRAG; ++f) wreg[f] = __builtin_bit_cast(bf16x8, wl[f * 64 + lane]);
    }
    auto wfrag = [&](int f) __attribute__((always_inline)) {
        if constexpr (WREG) return wreg[f];
        else return __builtin_bit_cast(bf16x8, wl[f * 64 + lane]);
    };

    // MAP forward: this lane's 16 MT slopes, for the whole launch (the map's register cost: 16 MT), and whether every slope
    // is a finite number >= 0 -- with t0 >= 0 and a finite map value >= 0 the threshold is then >= 0 (never NaN: no inf * 0)
    constexpr bool MAP_FWD = MAP && MODE != MODE_BWD;
    float tslr[MAP_FWD ? MT * 16 : 1];
    bool slope_any = false;
    if constexpr (MAP_FWD) {
        lane_channel_values<MT>(tslr, slope_s, h);
        slope_any = __ballot(lane < M && !(slope_s[lane] >= 0.0f && slope_s[lane] < __builtin_inff())) != 0ull;
    }

    const int xl = wxi * 32 + c;             // tile-local pixel column of this lane
    float *rsum = rsum_all + ((wxi & 1) + 2 * (wyi & 1)) * SLAB;
    const bool has_base = (MODE == MODE_FWD) || (MODE == MODE_BWD && p.zin != nullptr);
    const int hw4 = (int)HW * 4;

#pragma unroll 1
    for (int t = blockIdx.x; t < numTiles; t += gridDim.x) {
    const TileAt at = tile_decode(t, numTiles, p.tilesX, p.tilesY, p.rev);
    const int tile = at.tile, n = at.n;
    const int tx0 = at.txi * TW, ty0 = at.tyi * TH;
    const int x = tx0 + xl;
    if (MODE != MODE_BWD && tid < M) tau_s[tid] = p.tau[(size_t)n * M + tid];
    __syncthreads();                         // thin copies + tau of this tile are in place
    // next tile's thin loads fly during the GEMMs below: the registers (a run of 8, with DA two) stay live across the row
    // loop and are stored behind its barrier.  The reverse stage on 64 x 32 tiles (two waves per SIMD, 256 registers)
    // loads behind that barrier as it always did: its partner wave covers the wait, and loading ahead cost it scratch
    constexpr bool LOAD_AHEAD = MODE != MODE_BWD || WY == 2;
    if (LOAD_AHEAD) {
        stage_load(t + gridDim.x);
        if constexpr (DA) stage2_load(t + gridDim.x);
    }

    float ring[7][4];                        // row-direction col2im sums for halo rows yl .. yl+6, by (j & 3)
#pragma unroll
    for (int i = 0; i < 7; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) ring[i][j] = 0.0f;
    float tsum[MT * 16];                     // backward: per-lane partial threshold gradients
#pragma unroll
    for (int i = 0; i < MT * 16; ++i) tsum[i] = 0.0f;
    constexpr bool MAP_BWD = MAP && MODE == MODE_BWD;
    float tsum_w[MAP_BWD ? MT * 16 : 1];     // MAP backward: the same partials weighted by the map (dt[k,1,:])
    if constexpr (MAP_BWD) {
#pragma unroll
        for (int i = 0; i < MT * 16; ++i) tsum_w[i] = 0.0f;
    }
    // Reverse: one element's threshold partial, gt = -sign(z') * du.  Each element has its own accumulator, visited once per row
    // block in row-block order, so WHERE in the row block the update issues changes no bit.  TS_SHADOW: the updates of the 8
    // elements a synthesis k-step converts are written inside that k-step.  In the epilogue the compiler carried them round to
    // the head of the row loop, in front of the fat loads with the matrix pipe idle; from here it sinks them behind the last
    // synthesis MFMA (it does not interleave them), where the next block's loads are in flight (measured
    // together with PREFETCH below -- without it this form is the slower one).  A bf16-stored du_k sums the value
    // BEFORE its rounding, which the synthesis no longer has: those instances keep the update in the epilogue.  So do the map
    // modes: with a second set of partials live across the dA_k products their dA_k instances no longer fit 512 registers.
    constexpr bool TS_SHADOW = CDL_STAGE_TSUM_SHADOW && MODE == MODE_BWD && LOUT != LAY_BLK16 && !MAP;
    auto tsum_add = [&](int R, int v, float zz, unsigned sgb, float cm) __attribute__((always_inline)) {
        if CDL_DBG(p.dbg, 256) return;
        // zz where the sign bit of z' is set, -zz where it is clear: the complement of that bit, moved onto zz's sign (a shift, an
        // and, an xor; as a select it was a compare into a lane mask -- 32 scalar register pairs -- and a conditional move).
        // An off-support element is +0.0f and comes out -0.0f, as from the negation.
        const unsigned flip = (~sgb << (31 - (16 * R + v))) & 0x80000000u;
        const float gt = __builtin_bit_cast(float, __builtin_bit_cast(unsigned, zz) ^ flip);
        tsum[16 * R + v] += gt;
        if constexpr (MAP_BWD) tsum_w[16 * R + v] = fmaf(cm, gt, tsum_w[16 * R + v]);
    };
    // thresholds are >= 0 whenever project() runs (net.py:70); a negative one (3-D trainer, never projected) sends
    // the whole tile through the general shrinkage -- wave-uniform, so the common case pays 3 instructions per
    // element (u - clamp(u, -t, t)) instead of 10
    const bool tau_neg = (MODE != MODE_BWD && __ballot(lane < M && !(tau_s[lane] >= 0.0f)) != 0ull) || slope_any;   // negative OR NaN: the general, NaN-preserving form
    float taur[MT * 16];                     // forward: this lane's 16 MT thresholds
    if (MODE != MODE_BWD) lane_channel_values<MT>(taur, tau_s, h);

    // register v of accumulator tile R is channel 32R + 8(v>>2) + 4h + (v&3) of pixel column c
    const bool xok = x < p.W;
    const size_t img_in = lay_image_bytes<LIN>(M, p.H, p.W), img_out = lay_image_bytes<LOUT>(M, p.H, p.W);
    const __amdgpu_buffer_rsrc_t rs_in = uniform_rsrc(
        has_base ? (const char *)p.zin + (size_t)n * img_in : (const char *)p.zout, has_base ? img_in : 0);
    // bit 16R + v of the lane's words = register v of tile R: plane 2h holds [z != 0], plane 2h + 1 the sign bit
    unsigned *const map_n = p.map ? p.map + ((size_t)n * 4 + 2 * h) * HW : nullptr;
    const __amdgpu_buffer_rsrc_t rs_out = uniform_rsrc((const char *)p.zout + (size_t)n * img_out, img_out);
    const int lane_off = (int)((4 * h) * HW + x) * 4;
    // blocked layouts: block (y, xb) holds M/4 quads of [32 px][4 ch]; the lane's part is (h, c)
    const int XB = (p.W + 31) / 32, xb = (tx0 >> 5) + wxi;
    constexpr int EB_IN = LIN == LAY_BLK16 ? 8 : 16, EB_OUT = LOUT == LAY_BLK16 ? 8 : 16;
    const int lane_blk_in = (h * 32 + c) * EB_IN, lane_blk_out = (h * 32 + c) * EB_OUT;

    // -- fat inputs of the row block at image row y (valid: this lane's pixel is inside the image; else nothing is read)
    auto fat_loads = [&](int y, bool valid, int voff, int voff_in, float (&zc)[MT][16], u32x2 (&zr)[MT][4], unsigned &sup,
                         unsigned &sgb, float &cm) __attribute__((always_inline)) {
        if (MODE != MODE_FIRST && LIN == LAY_BLK16) {
            blk16_load_raw<MT>(zr, rs_in, voff_in);
        } else if (MODE != MODE_FIRST && CDL_DBG(p.dbg, 16)) {
#pragma unroll
            for (int R = 0; R < MT; ++R)
#pragma unroll
                for (int v = 0; v < 16; ++v) zc[R][v] = 0.25f;
        } else if (MODE != MODE_FIRST && LIN != LAY_NCHW) {
            blk_load<LIN, MT, CachePolicy::stage_fat_ld>(zc, rs_in, voff_in);
        } else if (MODE != MODE_FIRST) {
#pragma unroll
            for (int R = 0; R < MT; ++R)
#pragma unroll
                for (int v = 0; v < 16; ++v) {
                    const int soff = (32 * R + 8 * (v >> 2) + (v & 3)) * hw4;
                    zc[R][v] = buf_ld(rs_in, voff, soff);
                }
        }
        sup = 0; sgb = 0;                    // backward: support / sign words of this lane's pixel (0 outside)
        if (MODE == MODE_BWD && valid) {
            sup = map_n[(size_t)y * p.W + x];
            sgb = map_n[HW + (size_t)y * p.W + x];
        }
        cm = 0.0f;                           // MAP: the noise-level map at this lane's pixel (0 outside the image)
        if constexpr (MAP) {
            if (valid) cm = p.cmap[(size_t)n * HW + (size_t)y * p.W + x];
        }
    };
    // Reverse stage, one wave per SIMD: the fat inputs of row block b + 1 are issued behind the epilogue of block b -- its last
    // reader of these registers -- and land in the SAME registers while the dA_k products, the synthesis and the col2im of
    // block b run: no second landing set, no copies.  (Issued at the top of their own block they had the analysis GEMM's 24
    // MFMAs to arrive in, and with one wave per SIMD nobody else covers the rest of the wait.)  The first block of a tile is
    // loaded in front of the loop.
    // (Every other instance keeps its landing registers local to the row block, as they were: *_a are then one element.)
    constexpr bool PREFETCH = CDL_STAGE_PREFETCH && MODE == MODE_BWD && WY == 2;
    float zc_a[PREFETCH ? MT : 1][PREFETCH ? 16 : 1];
    u32x2 zr_a[PREFETCH ? MT : 1][PREFETCH ? 4 : 1];
    unsigned sup_a = 0, sgb_a = 0;
    float cm_a = 0.0f;
    auto fat_loads_ahead = [&](int b_, bool live) __attribute__((always_inline)) {
        if constexpr (PREFETCH) {
            const int y = ty0 + wyi * RB + b_;
            const bool valid = live && xok && (y < p.H);
            const int voff = valid ? lane_off + y * p.W * 4 : OOB;
            const int blk = (y * XB + xb) * (M / 4) * 32;
            fat_loads(y, valid, voff, LIN == LAY_NCHW ? voff : (valid ? blk * EB_IN + lane_blk_in : OOB), zc_a, zr_a, sup_a, sgb_a, cm_a);
        }
    };
    fat_loads_ahead(0, true);

#pragma unroll 1
    for (int b = 0; b < RB; ++b) {
        const int yl = wyi * RB + b;         // tile-local image row of this block
        const int y = ty0 + yl;
        const bool valid = xok && (y < p.H);
        const int voff = valid ? lane_off + y * p.W * 4 : OOB;
        const int blk = (y * XB + xb) * (M / 4) * 32;            // first [px][4 ch] slot of the block
        const int voff_in = LIN == LAY_NCHW ? voff : (valid ? blk * EB_IN + lane_blk_in : OOB);
        const int voff_st = (CDL_DBG(p.dbg, 1) || (MODE == MODE_BWD && p.drop_zout)) ? OOB : (LOUT == LAY_NCHW ? voff : (valid ? blk * EB_OUT + lane_blk_out : OOB));

        // -- fat inputs of this block, issued first: the analysis MFMAs below (and the partner
        //    wave on this SIMD) run while they are in flight
        float zc_b[PREFETCH ? 1 : MT][PREFETCH ? 1 : 16];
        u32x2 zr_b[PREFETCH ? 1 : MT][PREFETCH ? 1 : 4];         // LAY_BLK16: packed, decoded in the epilogue
        unsigned sup_b = 0, sgb_b = 0;
        float cm_b = 0.0f;
        float (&zc)[MT][16] = pick_ref<PREFETCH>(zc_a, zc_b);
        u32x2 (&zr)[MT][4] = pick_ref<PREFETCH>(zr_a, zr_b);
        unsigned &sup = PREFETCH ? sup_a : sup_b, &sgb = PREFETCH ? sgb_a : sgb_b;
        float &cm = PREFETCH ? cm_a : cm_b;
        if constexpr (!PREFETCH) fat_loads(y, valid, voff, voff_in, zc, zr, sup, sgb, cm);

        // -- im2col fragments of the thin input: 8 consecutive rows yl..yl+7 of column xl + j
        const int q = b & 3, e = yl - q;     // copy q is shifted up by q rows: 8-byte aligned window
        bf16x8 rh[4], rl[4];
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            const int col = xl + 2 * ks + h;
            rh[ks] = lds_window8(rt + (0 * 4 + q) * COPY + col * PITCH + e);
            if (PREC != 1) rl[ks] = lds_window8(rt + (1 * 4 + q) * COPY + col * PITCH + e);
        }

        __builtin_amdgcn_sched_barrier(0);   // phase fences: keep the scheduler from hoisting every LDS
                                             // weight read of the block to its top (register blow-up)
        // -- analysis-like GEMM (weights from LDS)
        // k-step outer, channel tile inner: the fragments of one k-step (all tiles) are read together, the products
        // alternate between the accumulator tiles, and the next k-step's fragments are read while they issue.  (Tile
        // outer / k-step inner was 12 dependent products per accumulator, each fragment read followed by a full LDS
        // wait: cdl_fusedg.hip's timeline study)
        f32x16 acc[MT];
        zero_tiles(acc);
        if CDL_DBG(p.dbg, 4) {
#pragma unroll
            for (int R = 0; R < MT; ++R) acc[R][0] = (float)rh[0][0] + (float)rl[1][1];
        } else {
            bf16x8 wh[2][MT], wlo[2][MT];
#pragma unroll
            for (int R = 0; R < MT; ++R) {
                wh[0][R] = wfrag(OFF_AH + R * 4);
                if (PREC != 1) wlo[0][R] = wfrag(OFF_AL + R * 4);
            }
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                const int cu = ks & 1, nx = cu ^ 1;
                if (ks + 1 < 4) {
#pragma unroll
                    for (int R = 0; R < MT; ++R) {
                        wh[nx][R] = wfrag(OFF_AH + R * 4 + ks + 1);
                        if (PREC != 1) wlo[nx][R] = wfrag(OFF_AL + R * 4 + ks + 1);
                    }
                }
                if (PREC != 1) {
#pragma unroll
                    for (int R = 0; R < MT; ++R) acc[R] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wlo[cu][R], rh[ks], acc[R], 0, 0, 0);
#pragma unroll
                    for (int R = 0; R < MT; ++R) acc[R] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wh[cu][R], rl[ks], acc[R], 0, 0, 0);
                    if (PREC == 2) {                                     // split4: the lo * lo term as well
#pragma unroll
                        for (int R = 0; R < MT; ++R) acc[R] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wlo[cu][R], rl[ks], acc[R], 0, 0, 0);
                    }
                }
#pragma unroll
                for (int R = 0; R < MT; ++R) acc[R] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wh[cu][R], rh[ks], acc[R], 0, 0, 0);
            }
        }

        __builtin_amdgcn_sched_barrier(0);
        // -- epilogue
        auto epilogue = [&](auto general_shrink) {
#pragma unroll
        for (int R = 0; R < MT; ++R)
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const int chl = 32 * R + 8 * (v >> 2) + (v & 3);        // + 4h folded into lane_off
                float zz;
                float zbase = 0.0f;
                if (MODE != MODE_FIRST) zbase = LIN == LAY_BLK16 ? blk16_decode(zr[R][v >> 2], v & 3) : zc[R][v];
                if (MODE == MODE_BWD) {
                    const bool on = (sup >> (16 * R + v)) & 1u;         // never for out-of-image lanes
                    zz = on ? zbase + acc[R][v] : 0.0f;
                    if constexpr (!TS_SHADOW) tsum_add(R, v, zz, sgb, cm);
                } else {
                    const float base = (MODE == MODE_FWD) ? zbase : 0.0f;
                    const float u = fmaf(p.sgn, acc[R][v], base);
                    // t >= 0: sign(u) relu(|u| - t) == u - clamp(u, -t, t) with the same rounding; NaN in u stays NaN
                    float tt = taur[16 * R + v];
                    if constexpr (MAP_FWD) tt = cdl_map_threshold(tt, cm, tslr[16 * R + v]);
                    const float st = decltype(general_shrink)::value ? cdl_shrink(u, tt)
                                                                     : u - __builtin_amdgcn_fmed3f(u, -tt, tt);
                    zz = CDL_DBG(p.dbg, 64) ? u : (valid ? st : 0.0f);
                }
                if (LOUT == LAY_BLK16) zz = bf16_round(zz);             // the code IS its stored value from here on
                if (LOUT == LAY_NCHW) buf_st(zz, rs_out, voff_st, chl * hw4);
                acc[R][v] = zz;
            }
        };
        // MAP: the clamp form needs every threshold of the row block >= 0 -- t0 and the slopes (tau_neg, per tile) and
        // the map values of this row block (a ballot: negative, NaN and infinite ones go to the general form)
        bool general = tau_neg;
        if constexpr (MAP_FWD) general = general || __ballot(!(cm >= 0.0f && cm < __builtin_inff())) != 0ull;
        if (general) epilogue(std::true_type{});   // wave-uniform
        else epilogue(std::false_type{});
        if (LOUT != LAY_NCHW) {
#pragma unroll
            for (int R = 0; R < MT; ++R)
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    blk_store4<LOUT, CachePolicy::stage_fat_st>(acc[R][4 * q], acc[R][4 * q + 1], acc[R][4 * q + 2], acc[R][4 * q + 3], rs_out,
                                     voff_st, 8 * R + 2 * q);
        }
        if (MODE != MODE_BWD && map_n) {      // training forward: 2 bits per code element for the reverse sweep
            unsigned ws = 0, wg = 0;
#pragma unroll
            for (int R = 0; R < MT; ++R)
#pragma unroll
                for (int v = 0; v < 16; ++v) {
                    const float zz = acc[R][v];
                    ws |= (zz != 0.0f ? 1u : 0u) << (16 * R + v);
                    wg |= (__builtin_bit_cast(unsigned, zz) >> 31) << (16 * R + v);
                }
            if (valid && !CDL_DBG(p.dbg, 1)) {
                map_n[(size_t)y * p.W + x] = ws;
                map_n[HW + (size_t)y * p.W + x] = wg;
            }
        }
        if constexpr (MAP_BWD) {
            // dL/dcmap[n,y,x] (+)= sum_m t1[m] g[m], g = -sign(z') * du as in tsum: the lane's 16 MT channels (du_k stands in
            // acc, the slopes come from LDS: two addresses per read, broadcast), plus the partner half's
            if (p.dcmap) {                   // launch-uniform
                float dcs = 0.0f;
#pragma unroll
                for (int R = 0; R < MT; ++R)
#pragma unroll
                    for (int qv = 0; qv < 4; ++qv) {
                        const float4 s4 = lane_channel_quad(slope_s, R, qv, h);
                        const float sl[4] = {s4.x, s4.y, s4.z, s4.w};
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            const int v = 4 * qv + e;
                            const float zz = acc[R][v];
                            dcs = fmaf(sl[e], ((sgb >> (16 * R + v)) & 1u) ? zz : -zz, dcs);
                        }
                    }
                dcs += __shfl_xor(dcs, 32, 64);
                if (h == 0 && valid) {
                    float *dst = p.dcmap + (size_t)n * HW + (size_t)y * p.W + x;
                    *dst = p.dc_add ? *dst + dcs : dcs;
                }
            }
        }
        const unsigned sgb_t = sgb;          // this block's sign words and map value, for the partials further down
        const float cm_t = cm;
        if constexpr (PREFETCH) {
            fat_loads_ahead(b + 1, b + 1 < RB);
            __builtin_amdgcn_sched_barrier(0);
        }
        if constexpr (DA) {
            // dA_k += du_k (x) im2col(r2) for this row block: k_wgrad2d's product with the fat operand taken from the
            // accumulator registers (register v of tile R = channel 32R + 8(v>>2) + 4h + (v&3) of pixel column c: the
            // layout its loads have) instead of from memory
            __bf16 *wimg = imgs2 + (size_t)wid * (MT * 2) * IMG_ELEMS;
            constexpr bool ALO = PREC != 1 && LOUT != LAY_BLK16;          // a bf16-stored du_k has no lo part
#pragma unroll
            for (int R = 0; R < MT; ++R)
#pragma unroll
                for (int qv = 0; qv < 4; ++qv)
                    wgrad_transpose_store<ALO>(wimg + (size_t)(R * 2) * IMG_ELEMS, qv, c, h, acc[R][4 * qv], acc[R][4 * qv + 1],
                                               acc[R][4 * qv + 2], acc[R][4 * qv + 3]);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            wgrad_products<MT, PREC, ALO>(dacc, wimg, thin2, yl, wxi, lane);
        }
        if ((MODE == MODE_BWD && !p.do_synth) || CDL_DBG(p.dbg, 2)) {           // no synthesis half: the partials here (launch-uniform)
            if constexpr (TS_SHADOW) {
#pragma unroll
                for (int R = 0; R < MT; ++R)
#pragma unroll
                    for (int v = 0; v < 16; ++v) tsum_add(R, v, acc[R][v], sgb_t, cm_t);
            }
            if CDL_DBG(p.dbg, 2) ring[0][0] += acc[0][0] + acc[MT - 1][15];
            continue;
        }

        __builtin_amdgcn_sched_barrier(0);
        // -- synthesis-like GEMM: the accumulator tiles are the B operand (k = channel) as they stand
        f32x16 D[2];
        zero_tiles(D);
        {
            // 16-channel k-steps q = 2R + s; the weight fragments of step q+1 (both tap tiles) are read while the products
            // of step q issue, and the products alternate between the two tap tiles
            bf16x8 bwh[2][2], bwl[2][2];
#pragma unroll
            for (int Rp = 0; Rp < 2; ++Rp) {
                bwh[0][Rp] = wfrag(OFF_BH + Rp * 2 * MT);
                if (PREC != 1) bwl[0][Rp] = wfrag(OFF_BL + Rp * 2 * MT);
            }
#pragma unroll
            for (int q = 0; q < 2 * MT; ++q) {
                const int R = q >> 1, s = q & 1, cu = q & 1, nx = cu ^ 1;
                if (q + 1 < 2 * MT) {
#pragma unroll
                    for (int Rp = 0; Rp < 2; ++Rp) {
                        bwh[nx][Rp] = wfrag(OFF_BH + Rp * 2 * MT + q + 1);
                        if (PREC != 1) bwl[nx][Rp] = wfrag(OFF_BL + Rp * 2 * MT + q + 1);
                    }
                }
                bf16x8 zh, zl;
#pragma unroll
                for (int jj = 0; jj < 8; ++jj) {
                    __bf16 hh, ll;
                    split_bf16(acc[R][8 * s + jj], hh, ll);
                    zh[jj] = hh;
                    if (PREC != 1 && LOUT != LAY_BLK16) zl[jj] = ll;      // a bf16-stored code has no lo part
                    if constexpr (TS_SHADOW) tsum_add(R, 8 * s + jj, acc[R][8 * s + jj], sgb_t, cm_t);
                }
                if (PREC != 1) {
#pragma unroll
                    for (int Rp = 0; Rp < 2; ++Rp) D[Rp] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bwl[cu][Rp], zh, D[Rp], 0, 0, 0);
                    if (LOUT != LAY_BLK16) {
#pragma unroll
                        for (int Rp = 0; Rp < 2; ++Rp) D[Rp] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bwh[cu][Rp], zl, D[Rp], 0, 0, 0);
                        if (PREC == 2) {
#pragma unroll
                            for (int Rp = 0; Rp < 2; ++Rp) D[Rp] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bwl[cu][Rp], zl, D[Rp], 0, 0, 0);
                        }
                    }
                }
#pragma unroll
                for (int Rp = 0; Rp < 2; ++Rp) D[Rp] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bwh[cu][Rp], zh, D[Rp], 0, 0, 0);
            }
        }

        __builtin_amdgcn_sched_barrier(0);
        // -- col2im, row direction: tap row i = 4Rp + (v>>2) of image row y lands on halo row yl + i;
        //    ring[i] collects halo row yl + i, ring[0] is complete after this block: flush and rotate
#pragma unroll
        for (int Rp = 0; Rp < 2; ++Rp)
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const int i = 4 * Rp + (v >> 2);
                if (i <= 6) ring[i][v & 3] += D[Rp][v];
            }
        // Column direction in registers (col2im_row), then ONE plain LDS store per lane: within a slab
        // every word is written by exactly one wave, once per tile (slabs are zeroed between tiles),
        // so no atomics and no read-modify-write are needed and the result is order-independent.
        {
            const float cs = col2im_row(ring[0], h);
            if (lane < 38 && !CDL_DBG(p.dbg, 32)) rsum[yl * RTW + 32 * wxi + lane] = cs;
        }
#pragma unroll
        for (int i = 0; i < 6; ++i)
#pragma unroll
            for (int jl = 0; jl < 4; ++jl) ring[i][jl] = ring[i + 1][jl];
#pragma unroll
        for (int jl = 0; jl < 4; ++jl) ring[6][jl] = 0.0f;
    }

    // ---- the 6 halo rows below the wave's last image row are still in the ring
    if (MODE != MODE_BWD || p.do_synth) {
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            const float cs = col2im_row(ring[i], h);
            if (lane < 38 && !CDL_DBG(p.dbg, 32)) rsum[(wyi * RB + RB + i) * RTW + 32 * wxi + lane] = cs;
        }
    }
    if (MODE == MODE_BWD && CDL_DBG(p.dbg, 256)) {           // timing only: the partials come out as zeros
        tacc_s[wid * 64 + lane] = 0.0f;
        if constexpr (MAP_BWD) tacc_w_s[wid * 64 + lane] = 0.0f;
    } else if (MODE == MODE_BWD) {
        tsum_to_lds<MT>(tsum, tacc_s + wid * 64, c, h);
        if constexpr (MAP_BWD) tsum_to_lds<MT>(tsum_w, tacc_w_s + wid * 64, c, h);   // the weighted sums: their own [wave][64]
    }
    __syncthreads();                         // every wave is done with the thin copies and the slabs
    if (!LOAD_AHEAD) stage_load(t + gridDim.x);
    if (MODE == MODE_BWD && tid < M) {
        float sacc = 0.0f;
#pragma unroll
        for (int w = 0; w < NW; ++w) sacc += tacc_s[w * 64 + tid];
        p.dtau[(size_t)tile * M + tid] = sacc;
        if constexpr (MAP_BWD) {
            float saccw = 0.0f;
#pragma unroll
            for (int w = 0; w < NW; ++w) saccw += tacc_w_s[w * 64 + tid];
            p.dtau_w[(size_t)tile * M + tid] = saccw;
        }
    }
    if CDL_DBG(p.dbg, 128) continue;
    if (MODE != MODE_BWD || p.do_synth) {    // patch out (fixed slab order), slabs re-zeroed for the next tile
        // One wave per SIMD: 16 bytes per access -- a slab is a whole number of them and so is a patch (p.patches is 16-byte
        // aligned), 2 passes over the 64 x 16 tile's slabs instead of 7.  (Two waves per SIMD: a dword, as before -- the
        // wider form added scratch to a 256-register reverse stage when tried.)  Element by element the same sum either way.
        typedef __attribute__((ext_vector_type(4))) float f32x4;
        using PV = std::conditional_t<WY == 2, f32x4, float>;
        constexpr int NV = SLAB * 4 / (int)sizeof(PV);
        static_assert(SLAB * 4 % sizeof(PV) == 0 && LDS_RT % sizeof(PV) == 0, "slabs and patches are whole vectors");
        PV *patch = reinterpret_cast<PV *>(p.patches + (size_t)tile * SLAB);
        PV *rs = reinterpret_cast<PV *>(rsum_all);
        for (int i = tid; i < NV; i += NT) {
            patch[i] = (rs[i] + rs[NV + i]) + (rs[2 * NV + i] + rs[3 * NV + i]);
            rs[i] = (PV)(0.0f); rs[NV + i] = (PV)(0.0f); rs[2 * NV + i] = (PV)(0.0f); rs[3 * NV + i] = (PV)(0.0f);
        }
    }
    stage_store();                           // next tile's thin copies (registers loaded in front of the row loop)
    if constexpr (DA) stage2_store();
    }   // tile loop
    if constexpr (DA) {
        // sum the waves through LDS (wave 0 stores, the others add in turn: fixed order, every lane owns its words) and
        // write this workgroup's partial in k_wgrad_reduce's layout, operator slot 0
        float *red = reinterpret_cast<float *>(smem);                           // [M][64] over the thin copies
        wgrad_wave_sum<MT, NW, 1>(dacc, red, 0, wid, tid, p.da_partial + (size_t)blockIdx.x * 2 * M * 64);
    }
}

// ------------------------------------------------------------------------------------------
// out[n,Y,X] = (mask ? mask : 1) * alpha * sum_{patches covering (Y,X)} patch - (sub ? sub : 0)
// A pixel is covered by its own tile's patch and, within HALO of a tile border, by the neighbour's across
// that border (and the diagonal one in a corner): at most 4 patches, visited in (tile row, tile column) order.
template <int WY>
__device__ __forceinline__ float patch_sum(const float *__restrict__ patches, int n, int Y, int X,
                                           int tilesX, int tilesY)
{
    constexpr int TH = Shape<WY>::TH, SLAB = Shape<WY>::SLAB;
    const int tyc = Y / TH, txc = X / TW;
    const int ly = Y - tyc * TH, lx = X - txc * TW;
    const int hx = (lx < HALO && txc > 0) ? -1 : ((lx >= TW - HALO && txc + 1 < tilesX) ? 1 : 0);
    const int vy = (ly < HALO && tyc > 0) ? -1 : ((ly >= TH - HALO && tyc + 1 < tilesY) ? 1 : 0);
    const float *own = patches + (((size_t)n * tilesY + tyc) * tilesX + txc) * SLAB + (ly + HALO) * RTW + lx + HALO;
    const ptrdiff_t dx = (ptrdiff_t)hx * (SLAB - TW), dy = (ptrdiff_t)vy * ((ptrdiff_t)tilesX * SLAB - TH * RTW);
    // the same pixel in the neighbour's patch: one tile over (SLAB words) and TW columns / TH rows back
    float sum = 0.0f;
    if (vy < 0) {
        if (hx < 0) sum += own[dy + dx];
        sum += own[dy];
        if (hx > 0) sum += own[dy + dx];
    }
    if (hx < 0) sum += own[dx];
    sum += own[0];
    if (hx > 0) sum += own[dx];
    if (vy > 0) {
        if (hx < 0) sum += own[dy + dx];
        sum += own[dy];
        if (hx > 0) sum += own[dy + dx];
    }
    return sum;
}

// ASM_ROWS image rows per thread: 4 for batches (fewer, fatter workgroups, 4 independent load chains), 1 for
// single small images where the launch is latency-bound and wants every workgroup it can get
template <int ASM_ROWS, int WY>
__global__ __launch_bounds__(256) void k_assemble(const float *__restrict__ patches,
                                                  const float *__restrict__ mask,
                                                  const float *__restrict__ sub, float alpha,
                                                  float *__restrict__ out, int N, int H, int W,
                                                  int tilesX, int tilesY, float *__restrict__ acc, int acc_add)
{
    // grid (ceil(W/256), ceil(H/ASM_ROWS), N): no runtime divisions (TW, TH are powers of two), rows coalesced
    const int X = blockIdx.x * 256 + threadIdx.x, n = blockIdx.z;
    if (X >= W) return;
#pragma unroll
    for (int j = 0; j < ASM_ROWS; ++j) {
        const int Y = blockIdx.y * ASM_ROWS + j;
        if (Y >= H) break;
        const size_t i = ((size_t)n * H + Y) * W + X;
        const float raw = patch_sum<WY>(patches, n, Y, X, tilesX, tilesY);
        if (acc) acc[i] = acc_add ? acc[i] + raw : raw;
        if (!out) continue;
        float sum = alpha * raw;
        if (mask) sum *= mask[i];
        if (sub) sum -= sub[i];
        out[i] = sum;
    }
}

// Batch form (W % 4 == 0): a thread owns 4 consecutive pixels of 2 rows -- the thin operands move as 16-byte vectors,
// a quarter of the threads issue half the memory instructions per pixel (same sums in the same order: bit-identical)
template <int WY>
__global__ __launch_bounds__(256) void k_assemble_v4(const float *__restrict__ patches,
                                                     const float *__restrict__ mask, const float *__restrict__ sub,
                                                     float alpha, float *__restrict__ out, int N, int H, int W,
                                                     int tilesX, int tilesY, float *__restrict__ accum, int acc_add)
{
    constexpr int TH = Shape<WY>::TH, SLAB = Shape<WY>::SLAB;
    // 4 consecutive pixels x 2 rows per thread.  The terms of a pixel are added in patch_sum's order (row above, own
    // row, row below; left neighbour, own tile, right neighbour), but the row candidates are wave-uniform branches and
    // the 8 loads of a patch row (4 own + up to 4 from the horizontal neighbour) are issued side by side instead of as
    // per-pixel dependent chains.  X is a multiple of 4 and TW of 64: the 4 pixels share their tile.
    const int X = (blockIdx.x * 64 + (threadIdx.x & 63)) * 4, n = blockIdx.z;
    if (X >= W) return;
    const int txc = X / TW, lx = X - txc * TW;
    int hx[4];
#pragma unroll
    for (int e = 0; e < 4; ++e)
        hx[e] = (lx + e < HALO && txc > 0) ? -1 : ((lx + e >= TW - HALO && txc + 1 < tilesX) ? 1 : 0);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int Y = (blockIdx.y * 4 + (threadIdx.x >> 6)) * 2 + j;
        if (Y >= H) break;
        const int tyc = Y / TH, ly = Y - tyc * TH;
        const int vy = (ly < HALO && tyc > 0) ? -1 : ((ly >= TH - HALO && tyc + 1 < tilesY) ? 1 : 0);        // uniform
        const float *own = patches + (((size_t)n * tilesY + tyc) * tilesX + txc) * SLAB + (ly + HALO) * RTW + lx + HALO;
        const ptrdiff_t dy = (ptrdiff_t)vy * ((ptrdiff_t)tilesX * SLAB - TH * RTW);
        float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        auto row = [&](ptrdiff_t off) {
            float a[4], b[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                a[e] = own[off + e];
                b[e] = hx[e] != 0 ? own[off + e + (ptrdiff_t)hx[e] * (SLAB - TW)] : 0.0f;
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (hx[e] < 0) acc[e] += b[e];
                acc[e] += a[e];
                if (hx[e] > 0) acc[e] += b[e];
            }
        };
        if (vy < 0) row(dy);
        row(0);
        if (vy > 0) row(dy);
        const size_t i = ((size_t)n * H + Y) * W + X;
        if (accum) {                                         // the unmasked, unscaled sum (data gradient)
            float4 a = make_float4(acc[0], acc[1], acc[2], acc[3]);
            if (acc_add) {
                const float4 o = *reinterpret_cast<const float4 *>(accum + i);
                a.x += o.x; a.y += o.y; a.z += o.z; a.w += o.w;
            }
            *reinterpret_cast<float4 *>(accum + i) = a;
        }
        if (!out) continue;
        float4 v = make_float4(alpha * acc[0], alpha * acc[1], alpha * acc[2], alpha * acc[3]);
        if (mask) {
            const float4 m = *reinterpret_cast<const float4 *>(mask + i);
            v.x *= m.x; v.y *= m.y; v.z *= m.z; v.w *= m.w;
        }
        if (sub) {
            const float4 sv = *reinterpret_cast<const float4 *>(sub + i);
            v.x -= sv.x; v.y -= sv.y; v.z -= sv.z; v.w -= sv.w;
        }
        *reinterpret_cast<float4 *>(out + i) = v;
    }
}

// ------------------------------------------------------------------------------------------
// Support / sign bit planes of a code tensor in the layout k_stage reads and writes them:
// map[n][2h + s][y][x], s = 0: bit (16R + v) = [z[n][ch][y][x] != 0], s = 1: its sign bit, with
// ch = 32R + 8(v>>2) + 4h + (v&3).  The training forward emits this map next to z_{k+1} (16 B per pixel
// against 256 B for M = 64), so the reverse stage reads 2 bits per element instead of the fat tensor.
// This kernel builds the same map from a tensor for callers that only hold z (tests, stepwise drivers).
__global__ __launch_bounds__(256) void k_support_map(const float *__restrict__ z, unsigned *__restrict__ map,
                                                     int N, int M, int H, int W)
{
    const size_t HW = (size_t)H * W;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)N * 2 * HW) return;
    const size_t pix = i % HW;
    const int h = (int)((i / HW) % 2), n = (int)(i / (2 * HW));
    unsigned ws = 0, wg = 0;
    for (int R = 0; R < M / 32; ++R)
        for (int v = 0; v < 16; ++v) {
            const int ch = 32 * R + 8 * (v >> 2) + 4 * h + (v & 3);
            const float zz = z[((size_t)n * M + ch) * HW + pix];
            ws |= (zz != 0.0f ? 1u : 0u) << (16 * R + v);
            wg |= (__builtin_bit_cast(unsigned, zz) >> 31) << (16 * R + v);
        }
    map[((size_t)n * 4 + 2 * h) * HW + pix] = ws;
    map[((size_t)n * 4 + 2 * h + 1) * HW + pix] = wg;
}

// ------------------------------------------------------------------------------------------
// Filter gradients on the matrix cores.
//   dw[ch][tap] = sum_px X[ch][px] * im2col(T)[tap][px]      (D = A * B with the PIXEL index as MFMA k)
// A operand = X[ch][k = 16 pixels of a row]: the fat tensor arrives with lanes = pixels (coalesced),
// so it is transposed through LDS: each lane stores its channels as packed bf16 into a [pixel][32 ch]
// image with 64-B rows (8-byte slots XOR-swizzled by (pixel>>1)&7: conflict-free stores) and the
// fragments come back through ds_read_b64_tr_b16 (conflict-free).
// B operand = im2col(T)[k = pixel][tap (i,j)] = T[y-3+i][x-3+j .. +7]: 8 consecutive columns of the
// one-channel halo tile; 4 column-shifted bf16 copies keep every such window 8-byte aligned.
// Workgroup = 8 waves: waves 0-3 reduce operator pair 0, waves 4-7 pair 1, each group covering a
// 64 x 16 pixel tile as 2 x 2 waves of 32 x 8; workgroups stride over the tiles keeping their
// [ch][tap] accumulators in registers; waves are then summed through LDS in a fixed order and one
// partial per workgroup is written.
struct WgradParams {
    const float *X[2];       // fat (N,M,H,W), nullptr = operator absent
    const float *T[2];       // thin (N,H,W)
    float *partial;          // (gridDim.x, 2, M, 64)
    int N, H, W, tilesX, tilesY, numTiles;
    int rev;                 // tiles from last to first
    int single;              // one operator (X[1] = X[0], T[1] = T[0]): both wave groups work on it, on alternate tiles; their
                             // two partial slots are added by k_wgrad_reduce
};

//   LAY: layout of the fat operands X[0], X[1] (LAY_*)
template <int MT, int PREC, int LAY>
__global__ __launch_bounds__(512) void k_wgrad2d(WgradParams p)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char dsm[];
    __bf16 *thin = reinterpret_cast<__bf16 *>(dsm);                            // [op][hl][s][TCOPY]
    __bf16 *imgs = reinterpret_cast<__bf16 *>(dsm + WG_THIN_BYTES);            // [wave][R][hl][IMG_ELEMS]
    constexpr int M = 32 * MT;
    // the wave index as a SCALAR: what hangs on it (operator pair, the pointers p.X[op] / p.T[op], tile and row indices)
    // then lives in SGPRs and comes from scalar loads.  As a per-lane value the compiler re-read p.X[op] through a
    // vector load inside the row loop and drained every outstanding fat load with vmcnt(0) in front of it
    const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int op = wid >> 2, wq = wid & 3;                                     // operator pair, wave in group
    const int wxi = wq & 1, wyi = wq >> 1;
    const int c = lane & 31, h = lane >> 5;
    const size_t HW = (size_t)p.H * p.W;
    __bf16 *wimg = imgs + (size_t)wid * (MT * 2) * IMG_ELEMS;
    f32x16 acc[MT][2];
#pragma unroll
    for (int R = 0; R < MT; ++R) zero_tiles(acc[R]);

    // zero the thin copies once: pad elements are read (into ignored tap columns) and must stay finite
    for (int i = tid; i < WG_THIN_BYTES / 16; i += 512) reinterpret_cast<uint4 *>(dsm)[i] = make_uint4(0, 0, 0, 0);

    const bool present = p.X[op] != nullptr;
    const int nsteps = p.single ? (p.numTiles + 1) / 2 : p.numTiles;
    const size_t img_b = lay_image_bytes<LAY>(M, p.H, p.W);
    const int hw4 = (int)HW * 4;

    // Software pipeline of the fat operand.  A wave used to load a row block, wait, convert, multiply, with nothing in
    // flight while it computed.  Now the loads run one row block ahead, into the other of two register sets (the row
    // loop alternates between them: no copies, and the wait in front of the conversions is for the older set only), the
    // first row block of the NEXT tile included -- tiles are a fixed stride -- so that they stay in flight across the
    // thin staging and its barriers.  Tiles, pixels and the order of the sums are what they were.  (The thin tile a tile
    // ahead as well, or no thin staging and no barriers at all, changed nothing measurable: DESIGN.md 5.2f.)
    struct Tile { bool active; int n, tx0, ty0; };
    auto tile_at = [&](int t0) {
        const int t = p.single ? 2 * t0 + op : t0;         // single operator: the wave groups take alternate tiles
        Tile q;
        q.active = present && t0 < nsteps && t < p.numTiles;                  // (per wave group)
        const TileAt at = tile_decode(t, p.numTiles, p.tilesX, p.tilesY, p.rev);
        q.n = q.active ? at.n : 0;
        q.tx0 = at.txi * TW; q.ty0 = at.tyi * GW_TH;
        return q;
    };
    // each group of 256 threads stages its own thin tile: all of a thread's elements are loaded (clamped addresses, no
    // branches) before any is converted: one at a time was seven dependent global-load latencies per 64 x 16 tile
    constexpr int NSW = (GW_RTH * RTW + 255) / 256;
    auto thin_load = [&](float (&tv)[NSW], const Tile &q) {
        const float *timg = p.T[op] + (size_t)q.n * HW;
#pragma unroll
        for (int k = 0; k < NSW; ++k) {
            const int i = (tid & 255) + k * 256;
            const int yy = i / RTW, xx = i % RTW;
            const int gy = q.ty0 - HALO + yy, gx = q.tx0 - HALO + xx;
            const bool ok = i < GW_RTH * RTW && gy >= 0 && gy < p.H && gx >= 0 && gx < p.W;
            const float v = timg[ok ? (size_t)gy * p.W + gx : 0];
            tv[k] = ok ? v : 0.0f;
        }
    };
    auto thin_write = [&](const float (&tv)[NSW]) {
#pragma unroll
        for (int k = 0; k < NSW; ++k) {
            const int i = (tid & 255) + k * 256;
            if (i >= GW_RTH * RTW) continue;
            const int yy = i / RTW, xx = i % RTW;
            __bf16 hh, ll;
            split_bf16(tv[k], hh, ll);
#pragma unroll
            for (int s = 0; s < 4; ++s)
                if (xx - s >= 0) {
                    thin[((op * 2 + 0) * 4 + s) * TCOPY + yy * TPITCH + xx - s] = hh;
                    if (PREC != 1) thin[((op * 2 + 1) * 4 + s) * TCOPY + yy * TPITCH + xx - s] = ll;
                }
        }
    };
    // ---- fat operand of one row block: registers (lanes = pixels); an inactive tile or an outside pixel loads zeros
    //      (offset beyond the descriptor: no memory access)
    struct Fat {
        float xv[MT][16];
        u32x2 xr[MT][4];                 // LAY_BLK16: the stored bf16 pairs ARE the hi fragments; there is no lo part
    };
    auto fat_load = [&](Fat &f, const Tile &q, int b) {
        const int x = q.tx0 + wxi * 32 + c, y = q.ty0 + wyi * RB + b;
        const bool valid = q.active && x < p.W && y < p.H;
        const __amdgpu_buffer_rsrc_t rs = uniform_rsrc((const char *)p.X[op] + (size_t)q.n * img_b, img_b);   // op: per wave group
        if (LAY == LAY_BLK16) {
            const int XB = (p.W + 31) / 32, xb = (q.tx0 >> 5) + wxi;
            blk16_load_raw<MT>(f.xr, rs, valid ? ((y * XB + xb) * (M / 4) * 32 + h * 32 + c) * 8 : OOB);
        } else if (LAY == LAY_BLK) {
            const int XB = (p.W + 31) / 32, xb = (q.tx0 >> 5) + wxi;
            blk_load<LAY_BLK, MT, CachePolicy::wgrad_fat_ld>(f.xv, rs, valid ? ((y * XB + xb) * (M / 4) * 32 + h * 32 + c) * 16 : OOB);
        } else {
            const int voff = valid ? (int)((4 * h) * HW + (size_t)y * p.W + x) * 4 : OOB;
#pragma unroll
            for (int R = 0; R < MT; ++R)
#pragma unroll
                for (int v = 0; v < 16; ++v)
                    f.xv[R][v] = buf_ld(rs, voff, (32 * R + 8 * (v >> 2) + (v & 3)) * hw4);
        }
    };
    // ---- one row block: bf16 hi/lo -> transposition images -> MFMAs against the thin tile's windows
    // op stays the wave-uniform scalar it is (above) where the base of its thin copies is formed
    constexpr bool ALO = PREC != 1 && LAY != LAY_BLK16;
    const __bf16 *thin_hi = thin + op * 8 * TCOPY;
    auto row_block = [&](const Fat &f, int b) {
#pragma unroll
        for (int R = 0; R < MT; ++R)
#pragma unroll
            for (int qv = 0; qv < 4; ++qv) {
                __bf16 *img = wimg + (size_t)(R * 2) * IMG_ELEMS;
                if (LAY == LAY_BLK16)
                    wgrad_transpose_store<false>(img, qv, c, h, __builtin_bit_cast(bf16x4, f.xr[R][qv]), bf16x4{});
                else
                    wgrad_transpose_store<ALO>(img, qv, c, h, f.xv[R][4 * qv], f.xv[R][4 * qv + 1], f.xv[R][4 * qv + 2],
                                               f.xv[R][4 * qv + 3]);
            }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        wgrad_products<MT, PREC, ALO>(acc, wimg, thin_hi, wyi * RB + b, wxi, lane);
    };

    static_assert(RB % 2 == 0, "the row loop alternates between two landing sets");
    Tile cur = tile_at(blockIdx.x);
    Fat fa, fb;
    fat_load(fa, cur, 0);
    for (int t0 = blockIdx.x; t0 < nsteps; t0 += gridDim.x) {
        const Tile nxt = tile_at(t0 + gridDim.x);
        __syncthreads();                                  // previous tile's readers are done
        if (cur.active) {
            float tv[NSW];
            thin_load(tv, cur);
            thin_write(tv);
        }
        __syncthreads();
#pragma unroll 1
        for (int b = 0; b < RB; b += 2) {
            fat_load(fb, cur, b + 1);
            if (cur.active) row_block(fa, b);
            if (b + 2 < RB) fat_load(fa, cur, b + 2);
            else fat_load(fa, nxt, 0);
            if (cur.active) row_block(fb, b + 1);
        }
        cur = nxt;
    }

    // ---- sum the four waves of each group through LDS (wave 0 stores, 1..3 add in turn: fixed
    //      order, every lane owns its own words) and write this workgroup's partial
    float *red = reinterpret_cast<float *>(dsm);                               // [2][M][64]
    wgrad_wave_sum<MT, 4, 2>(acc, red, op, wq, tid, p.partial + (size_t)blockIdx.x * 2 * M * 64);
}

// dw[ch][i'][j'] = alpha * sum_g partial[g][op][ch][8(i'+off) + (j'+off)].  32 outputs per workgroup,
// 32 strided partial sums each (1024 threads: the kernel is latency-bound, 16 loads per thread), combined
// in a fixed order (deterministic).
//   merge: both operator slots hold partials of ONE gradient (single-operator launches of k_wgrad2d): dw0 gets their sum
struct WgradReduce {
    const float *partial;    // (G, 2, M, 64)
    int G;
    float *dw0, *dw1;        // nullptr: operator absent
    float alpha0, alpha1;
    int merge;
};
__device__ __forceinline__ void wgrad_reduce_block(float (*red)[33], int block, const WgradReduce &q, int M, int P)
{
    const float *__restrict__ partial = q.partial;
    const int o = threadIdx.x & 31, part = threadIdx.x >> 5;
    const int t = block * 32 + o;
    const int per = M * P * P;
    const bool live = t < (q.merge ? per : 2 * per);
    float sum = 0.0f;
    int op = 0, r = 0;
    if (live) {
        op = t / per; r = t % per;
        const int ch = r / (P * P), ij = r % (P * P), off = (7 - P) / 2;
        const int tap = 8 * (ij / P + off) + (ij % P + off);
        for (int g = part; g < q.G; g += 32) {
            sum += partial[((size_t)(g * 2 + op) * M + ch) * 64 + tap];
            if (q.merge) sum += partial[((size_t)(g * 2 + 1) * M + ch) * 64 + tap];
        }
    }
    red[part][o] = sum;
    __syncthreads();
    if (part == 0 && live) {
        float *dw = op ? q.dw1 : q.dw0;
        if (dw) {
            float tot = 0.0f;
#pragma unroll
            for (int k = 0; k < 32; ++k) tot += red[k][o];
            dw[r] = (op ? q.alpha1 : q.alpha0) * tot;
        }
    }
}
inline int wgrad_reduce_blocks(const WgradReduce &q, int M, int P) { return ((q.merge ? 1 : 2) * M * P * P + 31) / 32; }

__global__ __launch_bounds__(1024) void k_wgrad_reduce(WgradReduce q, int M, int P)
{
    __shared__ float red[32][33];
    wgrad_reduce_block(red, blockIdx.x, q, M, P);
}

// dt0[m] = sum over workgroups; dt1[m] = sum_n c[n] * (sum over the workgroups of image n).  4 channels x 256
// row-strided partial sums per workgroup, tree-combined in a fixed order.
struct DtauReduce {
    const float *partial;    // (N * per_img, M)
    const float *c;
    float *dt0, *dt1;
    int N, per_img;
    const float *partial_w;  // nullable, never with c: the map-weighted partials (rows as partial's); dt1[m] = their sum
};
__device__ __forceinline__ void dtau_reduce_block(float (*r0)[4], float (*r1)[4], int block, const DtauReduce &q, int M)
{
    const float *__restrict__ partial = q.partial;
    const float *__restrict__ c = q.c;
    const float *__restrict__ pw = q.partial_w;
    const int mi = threadIdx.x & 3, part = threadIdx.x >> 2;
    const int m = block * 4 + mi;
    float a0 = 0.0f, a1 = 0.0f;
    const int rows = q.N * q.per_img;
    if (m < M && pw) {
        for (int row = part; row < rows; row += 256) {
            a0 += partial[(size_t)row * M + m];
            a1 += pw[(size_t)row * M + m];
        }
    } else if (m < M)
        for (int row = part; row < rows; row += 256) {
            const float v = partial[(size_t)row * M + m];
            a0 += v;
            if (c) a1 = fmaf(c[row / q.per_img], v, a1);
        }
    r0[part][mi] = a0;
    r1[part][mi] = a1;
    __syncthreads();
    for (int stride = 128; stride >= 1; stride >>= 1) {
        if (part < stride) { r0[part][mi] += r0[part + stride][mi]; r1[part][mi] += r1[part + stride][mi]; }
        __syncthreads();
    }
    if (part == 0 && m < M) { q.dt0[m] = r0[0][mi]; q.dt1[m] = r1[0][mi]; }
}

__global__ __launch_bounds__(1024) void k_dtau_reduce(DtauReduce q, int M)
{
    __shared__ float r0[256][4], r1[256][4];
    dtau_reduce_block(r0, r1, blockIdx.x, q, M);
}

// Every reduction of one reverse-sweep iteration in ONE launch: the three are tiny, latency-bound grids under which the
// device idles, so they run side by side on disjoint workgroup ranges -- [filter gradients a | filter gradients b |
// threshold gradients].  Each range runs the code of its stand-alone kernel: same sums in the same order.
struct SweepReduce {
    WgradReduce w[2];
    int wblocks[2];          // workgroups of each filter-gradient range (0: absent)
    DtauReduce t;
};
__global__ __launch_bounds__(1024) void k_sweep_reduce(SweepReduce q, int M, int P)
{
    __shared__ float sm[2 * 256 * 4];
    static_assert(sizeof(sm) >= 32 * 33 * sizeof(float), "k_wgrad_reduce's staging fits too");
    int block = blockIdx.x;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        if (block < q.wblocks[j]) {                          // (workgroup-uniform)
            wgrad_reduce_block(reinterpret_cast<float (*)[33]>(sm), block, q.w[j], M, P);
            return;
        }
        block -= q.wblocks[j];
    }
    dtau_reduce_block(reinterpret_cast<float (*)[4]>(sm), reinterpret_cast<float (*)[4]>(sm + 256 * 4), block, q.t, M);
}

inline bool fused_shape_ok(const cdl_geom *g)
{
    if (!cdl_geom_ok(g)) return false;
    if (g->C != 1 || g->D != 1 || g->Pd != 1 || g->sd != 1 || g->sh != 1 || g->sw != 1) return false;
    if (g->Ph != g->Pw || g->Ph > 7 || (g->Ph & 1) == 0 || g->ph != g->Ph / 2 || g->pw != g->Pw / 2) return false;
    if (g->M != 32 && g->M != 64) return false;
    if (blk_image_elems(g->M, g->H, g->W) * 4 >= ((size_t)1 << 31)) return false;   // per-image buffer descriptor range
    return true;
}

inline int debug_flags() { return cdl_opts().fused_debug; }

inline int tiles_x(const cdl_geom *g) { return (g->W + TW - 1) / TW; }
template <int WY> inline int tiles_y(const cdl_geom *g) { return (g->H + Shape<WY>::TH - 1) / Shape<WY>::TH; }

// `precision` argument of the entry points: bits 0-3 arithmetic (0 split-bf16 x3, 1 plain bf16, 2 split-bf16 x4: the
// lo * lo products as well -- exact fp32 products, for objectives that difference two forward passes), bit 4
// CDL_TILES_REVERSED, bits 5-6 layout of the fat INPUT(s), bits 7-8 layout of the fat OUTPUT (LAY_*)
struct Flags {
    int prec, rev, lin, lout;
    bool ok;
};
inline Flags parse_flags(int precision)
{
    Flags f;
    f.prec = precision & 15;
    f.rev = (precision >> 4) & 1;
    f.lin = (precision >> 5) & 3;
    f.lout = (precision >> 7) & 3;
    f.ok = (precision >> 9) == 0 && (f.prec == 0 || f.prec == 1 || f.prec == 2) && f.lin <= LAY_BLK16 && f.lout <= LAY_BLK16;
    return f;
}

template <int WY, int MT, int PREC, int MODE, int LIN, int LOUT>
int launch_stage_one(const FusedMapParams &p, dim3 grid, hipStream_t st)
{
    using G = Shape<WY>;
    constexpr int BASE = MODE & ~MODE_MAP;
    constexpr int LDS_MAP = MODE == MODE_BWD_MAP ? G::LDS_TACC : 0;        // the weighted [wave][64] sums, behind the rest
    // (blocked in, NCHW out) is the tangent sweep's last stage, which carries no dA ride: no such instance of it
    if constexpr (BASE == MODE_BWD && G::TH == GW_TH && !(LIN == LAY_BLK && LOUT == LAY_NCHW)) {
        if (p.r2) {                                          // the reverse stage that also accumulates dA_k
            if (int rc = cdl_ensure_dynamic_lds((const void *)k_stage<MT, PREC, MODE, LIN, LOUT, true, WY>, G::LDS_STAGE + G::LDS_DA + LDS_MAP)) return rc;
            k_stage<MT, PREC, MODE, LIN, LOUT, true, WY><<<grid, G::NT, G::LDS_STAGE + G::LDS_DA + LDS_MAP, st>>>(p);
            CDL_LAUNCH_CHECK();
            return 0;
        }
    }
    if (p.r2) return CDL_EUNSUPPORTED;
    if (int rc = cdl_ensure_dynamic_lds((const void *)k_stage<MT, PREC, MODE, LIN, LOUT, false, WY>, G::LDS_STAGE + LDS_MAP)) return rc;
    k_stage<MT, PREC, MODE, LIN, LOUT, false, WY><<<grid, G::NT, G::LDS_STAGE + LDS_MAP, st>>>(p);
    CDL_LAUNCH_CHECK();
    return 0;
}

// The layout pairs the sweeps and the step-wise entry points use: same layout on both sides, or NCHW on one
// side (z_K leaves a sweep as NCHW, a user gradient enters one as NCHW).  MODE_FIRST has no fat input.
// WY = 4 exists for sweeps with bf16 code storage only, and only the pairs such a sweep launches are instantiated:
//   FIRST (BLK16, BLK16) k = 0 of K > 1     FWD (BLK16, BLK16) 0 < k < K-1     BWD (NCHW, BLK16)  k = K-1
//   FIRST (NCHW, NCHW)   k = 0 of K = 1     FWD (BLK16, NCHW)  k = K-1 > 0     BWD (BLK16, BLK16) k < K-1
template <int WY, int MT, int PREC, int MODE>
int launch_stage_lay(const FusedMapParams &p, int lin, int lout, dim3 grid, hipStream_t st)
{
    if ((MODE & ~MODE_MAP) == MODE_FIRST) lin = lout;
#define CDL_LAY_CASE(a, b) if (lin == a && lout == b) return launch_stage_one<WY, MT, PREC, MODE, a, b>(p, grid, st)
    // A noise-level map: 64 x 16 tiles, split3 and fp32 storage only, in the layout pairs a default sweep launches --
    //   FIRST (NCHW, NCHW) (BLK, BLK)     FWD (NCHW, NCHW) (BLK, BLK) (BLK, NCHW)     BWD (NCHW, NCHW) (BLK, BLK) (NCHW, BLK)
    if constexpr ((MODE & MODE_MAP) != 0) {
        if constexpr (WY == 2 && PREC == 0) {
            CDL_LAY_CASE(LAY_NCHW, LAY_NCHW);
            CDL_LAY_CASE(LAY_BLK, LAY_BLK);
            if constexpr (MODE == MODE_FWD_MAP) CDL_LAY_CASE(LAY_BLK, LAY_NCHW);
            if constexpr (MODE == MODE_BWD_MAP) CDL_LAY_CASE(LAY_NCHW, LAY_BLK);
        }
        return CDL_EUNSUPPORTED;
    } else {
        if constexpr (WY == 2 || MODE == MODE_FIRST) CDL_LAY_CASE(LAY_NCHW, LAY_NCHW);
        if constexpr (WY == 2) CDL_LAY_CASE(LAY_BLK, LAY_BLK);
        CDL_LAY_CASE(LAY_BLK16, LAY_BLK16);
        if constexpr (MODE == MODE_FWD) {
            if constexpr (WY == 2) CDL_LAY_CASE(LAY_BLK, LAY_NCHW);
            CDL_LAY_CASE(LAY_BLK16, LAY_NCHW);
        }
        if constexpr (MODE == MODE_BWD) {
            if constexpr (WY == 2) CDL_LAY_CASE(LAY_NCHW, LAY_BLK);
            if constexpr (WY == 2) CDL_LAY_CASE(LAY_BLK, LAY_NCHW);      // the tangent sweep's last stage: zd_K leaves it as NCHW
            CDL_LAY_CASE(LAY_NCHW, LAY_BLK16);
        }
        return CDL_EUNSUPPORTED;
    }
#undef CDL_LAY_CASE
}

template <int WY, int MT, int PREC>
int launch_stage(const FusedMapParams &p, int mode, int lin, int lout, dim3 grid, hipStream_t st)
{
    if (mode == MODE_FWD) return launch_stage_lay<WY, MT, PREC, MODE_FWD>(p, lin, lout, grid, st);
    if (mode == MODE_FIRST) return launch_stage_lay<WY, MT, PREC, MODE_FIRST>(p, lin, lout, grid, st);
    if (mode == MODE_FWD_MAP) return launch_stage_lay<WY, MT, PREC, MODE_FWD_MAP>(p, lin, lout, grid, st);
    if (mode == MODE_FIRST_MAP) return launch_stage_lay<WY, MT, PREC, MODE_FIRST_MAP>(p, lin, lout, grid, st);
    if (mode == MODE_BWD_MAP) return launch_stage_lay<WY, MT, PREC, MODE_BWD_MAP>(p, lin, lout, grid, st);
    return launch_stage_lay<WY, MT, PREC, MODE_BWD>(p, lin, lout, grid, st);
}

// fn(MT, PREC) as integral constants, for M = 64 or 32 and the arithmetic f.prec (0 split3, 1 bf16, 2 split4): the one ladder
// over the template arguments every kernel of this file takes
template <class F>
int dispatch_mt_prec(int M, int prec, F &&fn)
{
    auto by_prec = [&](auto mt) {
        return prec == 0   ? fn(mt, std::integral_constant<int, 0>{})
               : prec == 1 ? fn(mt, std::integral_constant<int, 1>{})
                           : fn(mt, std::integral_constant<int, 2>{});
    };
    return M == 64 ? by_prec(std::integral_constant<int, 2>{}) : by_prec(std::integral_constant<int, 1>{});
}

// persistent workgroups: one per CU (most of its LDS each), striding over the tiles
int stage_grid(const cdl_geom *, const FusedMapParams &p)
{
    return (int)cdl_persistent_grid((size_t)p.N * p.tilesX * p.tilesY);
}

template <int WY>
int dispatch_stage(const cdl_geom *g, const FusedMapParams &p, int mode, const Flags &f, hipStream_t st)
{
    dim3 grid((unsigned)stage_grid(g, p));
    return dispatch_mt_prec(g->M, f.prec, [&](auto mt, auto prec) {
        return launch_stage<WY, decltype(mt)::value, decltype(prec)::value>(p, mode, f.lin, f.lout, grid, st);
    });
}

// persistent workgroups, one per CU (117 KB of LDS each: a CU holds one).  More than that -- it was 512 -- runs in
// rounds, and every round pays the LDS zero pass, a cold first tile, the cross-wave sum and 32 KB of partials again
int wgrad_grid(const cdl_geom *g)
{
    const size_t tiles = (size_t)g->N * tiles_x(g) * ((g->H + GW_TH - 1) / GW_TH);
    const size_t cus = (size_t)cdl_cu_count();
    return (int)(tiles < cus ? tiles : cus);
}

size_t wgrad_region_floats(const cdl_geom *g) { return (size_t)wgrad_grid(g) * 2 * g->M * 64; }

template <int MT, int PREC, int LAY>
int launch_wgrad_one(const WgradParams &p, int G, hipStream_t st)
{
    const size_t lds = (size_t)WG_THIN_BYTES + (size_t)8 * MT * 2 * IMG_ELEMS * 2;
    if (int rc = cdl_ensure_dynamic_lds((const void *)k_wgrad2d<MT, PREC, LAY>, (int)lds)) return rc;
    k_wgrad2d<MT, PREC, LAY><<<G, 512, lds, st>>>(p);
    CDL_LAUNCH_CHECK();
    return 0;
}

template <int MT, int PREC>
int launch_wgrad(const WgradParams &p, int lay, int G, hipStream_t st)
{
    if (lay == LAY_BLK) return launch_wgrad_one<MT, PREC, LAY_BLK>(p, G, st);
    if (lay == LAY_BLK16) return launch_wgrad_one<MT, PREC, LAY_BLK16>(p, G, st);
    return launch_wgrad_one<MT, PREC, LAY_NCHW>(p, G, st);
}

inline size_t larger(size_t a, size_t b) { return a > b ? a : b; }
template <int WY> inline size_t shape_tiles(const cdl_geom *g) { return (size_t)g->N * tiles_x(g) * tiles_y<WY>(g); }

// ---- the bodies behind the entry points that depend on the tile shape ------------------------------------
// what every stage launch sets, forward or reverse
template <int WY>
FusedMapParams stage_params(const cdl_geom *g, const Flags &f, const void *frags, float *patches)
{
    FusedMapParams p = {};
    p.rev = f.rev;
    p.frags = reinterpret_cast<const uint4 *>(frags);
    p.patches = patches; CDL_DBG_FIELD(p.dbg = debug_flags();)
    p.N = g->N; p.H = g->H; p.W = g->W;
    p.tilesX = tiles_x(g); p.tilesY = tiles_y<WY>(g);
    return p;
}

template <int WY>
int iter_fwd(const cdl_geom *g, const float *r, const float *zin, const float *tau, const void *frags, float sgn,
             float *zout, float *patches, unsigned *map_out, int precision, void *stream, const float *cmap = nullptr,
             const float *tslope = nullptr)
{
    if (!fused_shape_ok(g)) return CDL_EUNSUPPORTED;
    if (!r || !tau || !frags || !zout || !patches || zout == zin || !cmap != !tslope) return CDL_EINVAL;
    if (!cdl_aligned16(frags, patches)) return CDL_EUNSUPPORTED;     // library-sized buffers: 16-byte accesses (cdlnet_hip.h)
    const Flags f = parse_flags(precision);
    if (!f.ok) return CDL_EINVAL;
    if ((f.lin && !cdl_aligned16(zin)) || (f.lout && !cdl_aligned16(zout))) return CDL_EUNSUPPORTED;     // blocked codes: 16-byte accesses
    FusedMapParams p = stage_params<WY>(g, f, frags, patches);
    p.r = r; p.zin = zin; p.zout = zout; p.tau = tau; p.map = map_out;
    p.sgn = sgn; p.do_synth = 1;
    p.cmap = cmap; p.tslope = tslope;
    return dispatch_stage<WY>(g, p, (zin ? MODE_FWD : MODE_FIRST) | (cmap ? MODE_MAP : 0), f, S(stream));
}

int launch_wgrad_reduce(const cdl_geom *g, const WgradReduce &job, hipStream_t st)
{
    k_wgrad_reduce<<<wgrad_reduce_blocks(job, g->M, g->Ph), 1024, 0, st>>>(job, g->M, g->Ph);
    CDL_LAUNCH_CHECK();
    return 0;
}

// r2 != nullptr: the launch also produces dA = alpha * du_out (x) im2col(r2) (cdl_fused2d_wgrad's first operator pair, same
// arithmetic), through `workspace` (cdl_fused2d_wgrad_workspace_floats) -- one fat read of du_out less than the two-launch form
// defer: the reduction of the dA partials is not launched but described there
// A noise-level map in a reverse stage: the forward's map and slopes, dL/dcmap (nullable; add: accumulated, else written).
// With a map dtau_partial holds cdl_fused2d_dtau_partial_floats(g, 1) floats -- two arrays of cdl_fused2d_tiles(g) * M:
// the plain partials, then the weighted ones.
struct MapBwd {
    const float *cmap, *tslope;
    float *dcmap;
    int add;
};
inline float *weighted_partials(const cdl_geom *g, float *dtau_partial) { return dtau_partial + cdl_fused2d_tiles(g) * g->M; }

template <int WY>
int stage_bwd(const cdl_geom *g, const float *thin, const float *base, const unsigned *map, const void *frags,
              float *du_out, float *patches, float *dtau_partial, int do_synth, int precision, const float *r2,
              float alpha, float *dA, float *workspace, void *stream, WgradReduce *defer = nullptr, bool drop_out = false,
              const MapBwd &mb = MapBwd{})
{
    if (!fused_shape_ok(g)) return CDL_EUNSUPPORTED;
    if (!thin || !map || !frags || !du_out || !dtau_partial || du_out == base) return CDL_EINVAL;
    if (!mb.cmap != !mb.tslope || (mb.dcmap && !mb.cmap)) return CDL_EINVAL;
    if (!cdl_aligned16(frags, patches)) return CDL_EUNSUPPORTED;     // library-sized buffers: 16-byte accesses (cdlnet_hip.h)
    if (do_synth && !patches) return CDL_EINVAL;
    if (r2 && (!dA || !workspace)) return CDL_EINVAL;
    const Flags f = parse_flags(precision);
    if (!f.ok) return CDL_EINVAL;
    if ((f.lin && !cdl_aligned16(base)) || (f.lout && !cdl_aligned16(du_out))) return CDL_EUNSUPPORTED;  // blocked codes: 16-byte accesses
    FusedMapParams p = stage_params<WY>(g, f, frags, patches);
    p.r = thin; p.zin = base; p.map = const_cast<unsigned *>(map); p.zout = du_out; p.dtau = dtau_partial;
    p.sgn = 1.0f; p.do_synth = do_synth ? 1 : 0;
    p.r2 = r2; p.da_partial = workspace;
    p.drop_zout = drop_out ? 1 : 0;
    p.cmap = mb.cmap; p.tslope = mb.tslope; p.dcmap = mb.dcmap; p.dc_add = mb.add;
    p.dtau_w = mb.cmap ? weighted_partials(g, dtau_partial) : nullptr;
    int rc = dispatch_stage<WY>(g, p, mb.cmap ? MODE_BWD_MAP : MODE_BWD, f, S(stream));
    if (rc || !r2) return rc;
    const WgradReduce job = {workspace, stage_grid(g, p), dA, nullptr, alpha, 0.0f, 0};
    if (defer) { *defer = job; return 0; }                  // the sweep reduces it with the iteration's other sums
    return launch_wgrad_reduce(g, job, S(stream));
}

// k_wgrad2d into `workspace`; the reduction that finishes the gradient(s) is described in *job, not launched
int wgrad_partials(const cdl_geom *g, const float *X0, const float *T0, float alpha0, float *dw0,
                   const float *X1, const float *T1, float alpha1, float *dw1, float *workspace,
                   int precision, void *stream, WgradReduce *job)
{
    if (!fused_shape_ok(g)) return CDL_EUNSUPPORTED;
    if (!workspace || (!X0 && !X1)) return CDL_EINVAL;
    if ((X0 && (!T0 || !dw0)) || (X1 && (!T1 || !dw1))) return CDL_EINVAL;
    const Flags f = parse_flags(precision);
    if (!f.ok) return CDL_EINVAL;
    if (f.lin && !cdl_aligned16(X0, X1)) return CDL_EUNSUPPORTED;                                         // blocked codes: 16-byte accesses
    WgradParams p = {};
    p.rev = f.rev;
    p.X[0] = X0; p.T[0] = T0; p.X[1] = X1; p.T[1] = T1;
    p.single = (X0 != nullptr) != (X1 != nullptr);
    if (p.single) {                                         // one gradient: both wave groups on it
        if (!X0) { X0 = X1; T0 = T1; alpha0 = alpha1; dw0 = dw1; X1 = nullptr; }
        p.X[0] = p.X[1] = X0; p.T[0] = p.T[1] = T0;
    }
    p.partial = workspace;
    p.N = g->N; p.H = g->H; p.W = g->W;
    p.tilesX = tiles_x(g); p.tilesY = (g->H + GW_TH - 1) / GW_TH;
    p.numTiles = p.N * p.tilesX * p.tilesY;
    int G = wgrad_grid(g);
    if (p.single && G > (p.numTiles + 1) / 2) G = (p.numTiles + 1) / 2;
    const int rc = dispatch_mt_prec(g->M, f.prec, [&](auto mt, auto prec) {
        return launch_wgrad<decltype(mt)::value, decltype(prec)::value>(p, f.lin, G, S(stream));
    });
    if (rc) return rc;
    *job = WgradReduce{workspace, G, X0 ? dw0 : nullptr, X1 ? dw1 : nullptr, alpha0, alpha1, p.single};
    return 0;
}

template <int WY>
int assemble(const cdl_geom *g, const float *patches, const float *mask, const float *sub, float alpha, float *out,
             float *acc, int acc_add, void *stream)
{
    if (!fused_shape_ok(g)) return CDL_EUNSUPPORTED;
    if (!patches || (!out && !acc)) return CDL_EINVAL;
    const int tx = tiles_x(g), ty = tiles_y<WY>(g);
    if ((size_t)g->N * g->H * g->W >= ((size_t)1 << 20) && cdl_assemble16(g->W, out, mask, sub, acc)) {
        dim3 grid((unsigned)((g->W + 255) / 256), (unsigned)((g->H + 7) / 8), (unsigned)g->N);
        k_assemble_v4<WY><<<grid, 256, 0, S(stream)>>>(patches, mask, sub, alpha, out, g->N, g->H, g->W, tx, ty, acc, acc_add);
        CDL_LAUNCH_CHECK();
    } else if ((size_t)g->N * g->H * g->W >= ((size_t)1 << 20)) {
        dim3 grid((unsigned)((g->W + 255) / 256), (unsigned)((g->H + 3) / 4), (unsigned)g->N);
        k_assemble<4, WY><<<grid, 256, 0, S(stream)>>>(patches, mask, sub, alpha, out, g->N, g->H, g->W, tx, ty, acc, acc_add);
        CDL_LAUNCH_CHECK();
    } else {
        dim3 grid((unsigned)((g->W + 255) / 256), (unsigned)g->H, (unsigned)g->N);
        k_assemble<1, WY><<<grid, 256, 0, S(stream)>>>(patches, mask, sub, alpha, out, g->N, g->H, g->W, tx, ty, acc, acc_add);
        CDL_LAUNCH_CHECK();
    }
    return 0;
}

/* ---- optional per-kernel timing inside the sweeps (HIP events on the launch stream) -------------------
 * bench.py turns it on for a few steps to report the in-step average duration of the three fat kernels
 * (isolated re-launches of one kernel miss the cache state the step leaves behind).  Off: no events. */
// Process-wide and mutex-guarded: the one piece of state of this file, used by bench.py only.  Events are
// recorded on whichever stream the timed sweep runs on; pairs of different devices are kept apart by the
// device they were created on (an event can only be recorded on its own device's streams).
struct TimingState {
    std::mutex mu;
    std::atomic<bool> on{false};
    struct Pair { hipEvent_t start, stop; int cls, dev; };
    std::vector<Pair> pairs;               // in launch order; class 0 forward stage (k >= 1), 1 reverse stage,
                                           // 2 filter gradients, 3 first forward stage (k = 0: no fat read)
    std::vector<std::pair<hipEvent_t, int>> spare;     // recycled events with their device
};
TimingState g_timing;

struct TimingScope {
    hipStream_t st;
    hipEvent_t stop = nullptr;
    TimingScope(int c, hipStream_t s) : st(s)
    {
        if (!g_timing.on.load(std::memory_order_relaxed)) return;
        std::lock_guard<std::mutex> lk(g_timing.mu);
        const int dev = cdl_current_device();
        hipEvent_t ev[2] = {nullptr, nullptr};
        for (int i = 0; i < 2; ++i) {
            for (size_t k = 0; k < g_timing.spare.size() && !ev[i]; ++k)
                if (g_timing.spare[k].second == dev) {
                    ev[i] = g_timing.spare[k].first;
                    g_timing.spare.erase(g_timing.spare.begin() + k);
                }
            if (!ev[i] && hipEventCreate(&ev[i]) != hipSuccess) return;
        }
        (void)hipEventRecord(ev[0], st);
        stop = ev[1];
        g_timing.pairs.push_back({ev[0], ev[1], c, dev});
    }
    ~TimingScope()
    {
        if (stop) (void)hipEventRecord(stop, st);
    }
};

/* ---- whole sweeps: every launch of a forward / reverse pass enqueued from one C call ----------------
 * Snake order: consecutive fat launches walk the tiles in opposite directions, so each one starts on
 * the bytes the previous one touched last, which are still in the 256 MiB Infinity Cache (it holds
 * the last ~256 MiB loaded or stored).  Tile results do not depend on the order; only the filter
 * gradients' per-workgroup partial sums are grouped differently.  CDL_FUSED_SNAKE=0 turns it off. */
// fragments of K (analysis-like, synthesis-like) pairs, pair k at frags + k * cdl_fused2d_frag_bytes(M)
int prep_pairs(const float *const *w1, const float *const *w2, int K, int shift2, void *frags, int M, int P,
               hipStream_t st)
{
    if (!cdl_aligned16(frags)) return CDL_EUNSUPPORTED;      // the library-sized fragment buffer is written 16 bytes at a time (cdlnet_hip.h)
    const int MT = M / 32, threads = 8 * MT * 64;
    const int frag_uint4 = (int)(cdl_fused2d_frag_bytes(M) / 16);
    for (int k0 = 0; k0 < K; k0 += PREP_BATCH) {
        PrepBatch b;
        const int nb = cdl_pair_batch(&b, w1, w2, K, shift2, k0);       // forward: (A_k, B_{k+1 mod K});  backward: (B_{k+1 mod K}, A_k)
        dim3 grid((unsigned)((threads + 255) / 256), (unsigned)nb);
        k_prep_batch<<<grid, 256, 0, st>>>(b, reinterpret_cast<uint4 *>(frags) + (size_t)k0 * frag_uint4, frag_uint4, MT, P);
        CDL_LAUNCH_CHECK();
    }
    return 0;
}

int snake_enabled() { return cdl_opts().fused_snake; }

// Sweeps: CDL_LAYOUT_IN(L) in `precision` selects the layout L of the tensors that stay inside the sweeps --
// z_1 .. z_{K-1} (z[0..K-2]) and the du ping-pong buffers; z_K (z[K-1]) and g_z are always NCHW fp32.
// The C entry points have checked the arguments and picked WY from L.
template <int WY>
int forward_sweep(const cdl_geom *g, int K, const float *yp, const float *mask, const float *tau,
                  const float *const *wA, const float *const *wB, float *const *z, float *const *r,
                  unsigned *const *maps, float *xp, void *frags, float *patches, const Flags &f, void *stream,
                  const float *cmap = nullptr, const float *tslope = nullptr)
{
    const size_t nm = (size_t)g->N * g->M;
    const int L = f.lin;
    int rc = prep_pairs(wA, wB, K, 1, frags, g->M, g->Ph, S(stream));       // (A_k, B_{k+1}) for every k, one launch
    if (rc) return rc;
    return cdl_forward_order_sweep(
        K, frags, cdl_fused2d_frag_bytes(g->M), yp, mask, yp, 1.0f, r, xp, snake_enabled(), L, LAY_NCHW,
        [&](int k, const void *fk, const float *thin, bool reversed, int, int lay_out) {
            TimingScope ts(k ? 0 : 3, S(stream));               // (the input layout is L at k = 0 too, where no code is read)
            return iter_fwd<WY>(g, thin, k ? z[k - 1] : nullptr, tau + k * nm, fk, k ? -1.0f : 1.0f, z[k], patches, maps ? maps[k] : nullptr,
                                f.prec | CDL_LAYOUT_IN(L) | CDL_LAYOUT_OUT(lay_out) | (reversed ? CDL_TILES_REVERSED : 0), stream,
                                cmap, cmap ? tslope + (size_t)k * g->M : nullptr);
        },
        [&](const float *m, const float *sub, float alpha, float *out) {
            return assemble<WY>(g, patches, m, sub, alpha, out, nullptr, 0, stream);
        });
}

template <int WY>
int backward_sweep(const cdl_geom *g, int K, const float *yp, const float *mask, const float *c,
                   const float *const *wA, const float *const *wB, const float *const *z,
                   const float *const *r, const unsigned *const *maps, const float *g_xp,
                   const float *g_z, float *const *dA,
                   float *const *dB, float *dt, float *du0, float *du1, float *q, void *frags,
                   float *patches, float *dtau_partial, float *wgrad_ws, const Flags &f, float *dyp,
                   float *dtau, void *stream, const float *cmap = nullptr, const float *tslope = nullptr,
                   float *dcmap = nullptr)
{
    const int M = g->M;
    float *du[2] = {du0, du1};
    const int L = f.lin;
    // the forward's last launch ran in direction (K-1)&1: stages take that one, filter gradients the other
    const int sdir = snake_enabled() ? (((K - 1) & 1) ? CDL_TILES_REVERSED : 0) : 0;
    const int wdir = snake_enabled() ? (sdir ^ CDL_TILES_REVERSED) : 0;
    const int sprec = f.prec | sdir, wprec = f.prec | wdir;
    int rc = cdl_fused2d_wgrad(g, z[K - 1], g_xp, 1.0f, dB[0], nullptr, nullptr, 0.0f, nullptr, wgrad_ws,
                               wprec, stream);                           // dB_0 = z_K (x) dL/d(D z_K); z_K is NCHW
    if (rc) return rc;
    const float *thin = g_xp, *base = g_z;
    const size_t fb = cdl_fused2d_frag_bytes(M);
    rc = prep_pairs(wB, wA, K, 0, frags, M, g->Ph, S(stream));               // (B_{k+1}, A_k) for every k, one launch
    if (rc) return rc;
    // One reduction launch per iteration (k_sweep_reduce), after the iteration's last fat kernel: dA_k (the stage's
    // partials, first region of the workspace), dB_k (k_wgrad2d's, second region) and the threshold gradients of k.
    // dtau_partial is next written by stage k-1, behind that launch in stream order.
    float *ws_a = wgrad_ws, *ws_b = wgrad_ws + wgrad_region_floats(g);
    const int per_img = tiles_x(g) * tiles_y<WY>(g);         // dtau_partial rows: [n][tile][m]
    for (int k = K - 1, flip = 0; k >= 0; --k, flip ^= 1) {
        const void *fk = static_cast<const char *>(frags) + (size_t)k * fb;
        float *duk = du[flip];
        // dA_k = -du_k (x) r_k (k = 0: du_0 (x) yp) rides in the reverse stage, which has du_k in its registers: du_k is
        // read once (by stage k-1), not twice -- 5.1 fat passes per iteration instead of 6.1 (CDL_FUSED_DA=0: the two-launch
        // form, for A/B runs).  On 64 x 32 tiles it does not: k_wgrad2d takes both operand pairs
        const bool ride = Shape<WY>::TH == GW_TH && cdl_opts().fused_da;
        SweepReduce red = {};
        {
            // with the ride nobody reads du_0 from memory (dA_0 and the patches for dyp come out of the stage's registers, and
            // no stage follows): the last stage does not write it -- one fat write per sweep less
            TimingScope ts(1, S(stream));
            rc = stage_bwd<WY>(g, thin, base, maps[k], fk, duk, patches, dtau_partial, k >= 1 || dyp,
                               sprec | CDL_LAYOUT_IN(k == K - 1 ? LAY_NCHW : L) | CDL_LAYOUT_OUT(L),
                               ride ? (k >= 1 ? r[k - 1] : yp) : nullptr, k >= 1 ? -1.0f : 1.0f, dA[k], ws_a, stream, &red.w[0],
                               ride && k == 0,
                               MapBwd{cmap, cmap ? tslope + (size_t)k * M : nullptr, dcmap, k < K - 1});   // dcmap: = at k = K-1, += after
        }
        if (rc) return rc;
        if (ride) red.wblocks[0] = wgrad_reduce_blocks(red.w[0], M, g->Ph);
        red.t = DtauReduce{dtau_partial, c, dt + (size_t)k * 2 * M, dt + (size_t)k * 2 * M + M, g->N, per_img,
                           cmap ? weighted_partials(g, dtau_partial) : nullptr};
        if (dtau) {
            rc = cdl_dtau_per_sample(dtau_partial, g->N, M, per_img, (size_t)per_img * M, 1, M, dtau + (size_t)k * g->N * M, stream);
            if (rc) return rc;
        }
        if (k == 0 && dyp) {                                    // u_0 = A_0 yp: dyp += A_0^T du_0 (no q at k = 0)
            rc = assemble<WY>(g, patches, nullptr, nullptr, 1.0f, nullptr, dyp, K > 1, stream);
            if (rc) return rc;
        }
        if (k >= 1) {
            // q_k = -mask A_k^T du_k; with dyp the same sum, unmasked, goes to dyp (= at k = K-1, += after)
            rc = assemble<WY>(g, patches, mask, nullptr, -1.0f, q, dyp, k < K - 1, stream);
            if (rc) return rc;
            {
                TimingScope ts(2, S(stream));
                rc = ride ? wgrad_partials(g, z[k - 1], q, 1.0f, dB[k], nullptr, nullptr, 0.0f, nullptr, ws_b,
                                           wprec | CDL_LAYOUT_IN(L), stream, &red.w[1])
                          : wgrad_partials(g, duk, r[k - 1], -1.0f, dA[k], z[k - 1], q, 1.0f, dB[k], ws_b,
                                           wprec | CDL_LAYOUT_IN(L), stream, &red.w[1]);
            }
            thin = q;
        } else if (!ride) {
            rc = wgrad_partials(g, duk, yp, 1.0f, dA[0], nullptr, nullptr, 0.0f, nullptr, ws_b, wprec | CDL_LAYOUT_IN(L), stream,
                                &red.w[1]);
        }
        if (rc) return rc;
        if (k >= 1 || !ride) red.wblocks[1] = wgrad_reduce_blocks(red.w[1], M, g->Ph);
        k_sweep_reduce<<<red.wblocks[0] + red.wblocks[1] + (M + 3) / 4, 1024, 0, S(stream)>>>(red, M, g->Ph);
        CDL_LAUNCH_CHECK();
        base = duk;
    }
    return 0;
}

// Forward-mode tangent sweep at the primal's supports.  The reverse stage computes
// [z' != 0] * (base + corr(thin; W1)) and the patches of W2^T of it from ANY prepared pair: with the forward's pairs
// (A_k, B_{k+1}), base = zd_k, thin = -rd_k and the primal's bit map of z_{k+1} it is one tangent iteration, and the assemble
// with alpha = -1 and sub = -vp hands the next stage its thin operand -rd_{k+1} = vp - mask B_{k+1} zd_{k+1}.  The stage's
// threshold partials (dtau_partial) are never reduced.
template <int WY>
int tangent_sweep(const cdl_geom *g, int K, const float *vp, const float *nvp, const float *mask,
                  const float *const *wA, const float *const *wB, const unsigned *const *maps, float *const *zd,
                  float *const *nrd, float *xdp, void *frags, float *patches, float *dtau_partial, const Flags &f,
                  void *stream)
{
    int rc = prep_pairs(wA, wB, K, 1, frags, g->M, g->Ph, S(stream));       // (A_k, B_{k+1}), the forward's pairs
    if (rc) return rc;
    return cdl_forward_order_sweep(
        K, frags, cdl_fused2d_frag_bytes(g->M), vp, mask, nvp, -1.0f, nrd, xdp, snake_enabled(), f.lin, LAY_NCHW,
        [&](int k, const void *fk, const float *thin, bool reversed, int lay_in, int lay_out) {
            return stage_bwd<WY>(g, thin, k ? zd[k - 1] : nullptr, maps[k], fk, zd[k], patches, dtau_partial, 1,
                                 f.prec | CDL_LAYOUT_IN(lay_in) | CDL_LAYOUT_OUT(lay_out) | (reversed ? CDL_TILES_REVERSED : 0),
                                 nullptr, 0.0f, nullptr, nullptr, stream);
        },
        [&](const float *m, const float *sub, float alpha, float *out) {
            return assemble<WY>(g, patches, m, sub, alpha, out, nullptr, 0, stream);
        });
}

}  // namespace

// The C ABI.  Step-wise entry points always work on 64 x 16 tiles; the two sweeps pick the shape from the code layout.
extern "C" {

int cdl_fused2d_supported(const cdl_geom *g) { return fused_shape_ok(g) ? 1 : 0; }

size_t cdl_fused2d_frag_bytes(int M) { return (size_t)2 * (M / 32) * 8 * 64 * 16; }

// (buffers a caller sizes with these serve sweeps on either tile shape: the larger of the two needs)
// floats of a reverse stage's dtau_partial: one (tiles, M) array, and with a noise-level map the weighted one behind it
size_t cdl_fused2d_dtau_partial_floats(const cdl_geom *g, int with_map)
{
    return (with_map ? 2 : 1) * cdl_fused2d_tiles(g) * (fused_shape_ok(g) ? (size_t)g->M : 0);
}

size_t cdl_fused2d_patch_floats(const cdl_geom *g)
{
    if (!fused_shape_ok(g)) return 0;
    return larger(shape_tiles<2>(g) * Shape<2>::SLAB, shape_tiles<4>(g) * Shape<4>::SLAB);
}

size_t cdl_fused2d_tiles(const cdl_geom *g)
{
    if (!fused_shape_ok(g)) return 0;
    return larger(shape_tiles<2>(g), shape_tiles<4>(g));
}

int cdl_fused2d_prep(const float *wA, const float *wB, void *frags, int M, int P, void *stream)
{
    if (!wA || !wB || !frags || (M != 32 && M != 64) || P < 1 || P > 7 || !(P & 1)) return CDL_EINVAL;
    if (!cdl_aligned16(frags)) return CDL_EUNSUPPORTED;      // a library-sized fragment buffer: 16-byte accesses (cdlnet_hip.h)
    const int MT = M / 32, threads = 8 * MT * 64;
    k_prep<<<(threads + 255) / 256, 256, 0, S(stream)>>>(wA, wB, reinterpret_cast<uint4 *>(frags), MT, P);
    CDL_LAUNCH_CHECK();
    return 0;
}

size_t cdl_fused2d_code_bytes(const cdl_geom *g, int layout)
{
    if (!fused_shape_ok(g) || layout < 0 || layout > LAY_BLK16) return 0;
    const size_t per = layout == LAY_NCHW ? lay_image_bytes<LAY_NCHW>(g->M, g->H, g->W)
                     : layout == LAY_BLK ? lay_image_bytes<LAY_BLK>(g->M, g->H, g->W)
                                         : lay_image_bytes<LAY_BLK16>(g->M, g->H, g->W);
    return (size_t)g->N * per;
}

size_t cdl_fused2d_map_words(const cdl_geom *g)
{
    if (!fused_shape_ok(g)) return 0;
    return (size_t)g->N * 4 * g->H * g->W;
}

int cdl_fused2d_support_map(const cdl_geom *g, const float *z, unsigned *map, void *stream)
{
    if (!fused_shape_ok(g)) return CDL_EUNSUPPORTED;
    if (!z || !map) return CDL_EINVAL;
    const size_t total = (size_t)g->N * 2 * g->H * g->W;
    k_support_map<<<(unsigned)((total + 255) / 256), 256, 0, S(stream)>>>(z, map, g->N, g->M, g->H, g->W);
    CDL_LAUNCH_CHECK();
    return 0;
}

int cdl_fused2d_iter_fwd(const cdl_geom *g, const float *r, const float *zin, const float *tau,
                         const void *frags, float sgn, float *zout, float *patches, unsigned *map_out,
                         int precision, const float *cmap, const float *tslope, void *stream)
{
    return iter_fwd<2>(g, r, zin, tau, frags, sgn, zout, patches, map_out, precision, stream, cmap, tslope);
}

int cdl_fused2d_stage_bwd(const cdl_geom *g, const float *thin, const float *base, const unsigned *map,
                          const void *frags, float *du_out, float *patches, float *dtau_partial, int do_synth,
                          const float *r2, float alpha, float *dA, float *workspace, int precision, const float *cmap,
                          const float *tslope, float *dcmap, int dcmap_add, void *stream)
{
    if (!r2 != !dA || !r2 != !workspace) return CDL_EINVAL;     // the filter gradient: all three set, or none
    return stage_bwd<2>(g, thin, base, map, frags, du_out, patches, dtau_partial, do_synth, precision, r2, alpha, dA, workspace,
                        stream, nullptr, false, MapBwd{cmap, tslope, dcmap, dcmap_add});
}

int cdl_fused2d_dtau_reduce(const cdl_geom *g, const float *dtau_partial, const float *c, float *dt0, float *dt1,
                            float *dtau_n, const float *dtau_partial_w, void *stream)
{
    if (!fused_shape_ok(g)) return CDL_EUNSUPPORTED;
    if (!dtau_partial || !dt0 || !dt1 || (c && dtau_partial_w)) return CDL_EINVAL;
    const int per_img = tiles_x(g) * tiles_y<2>(g);          // partial rows: [n][tile][m]
    const DtauReduce job = {dtau_partial, c, dt0, dt1, g->N, per_img, dtau_partial_w};
    k_dtau_reduce<<<(g->M + 3) / 4, 1024, 0, S(stream)>>>(job, g->M);
    CDL_LAUNCH_CHECK();
    if (!dtau_n) return 0;
    return cdl_dtau_per_sample(dtau_partial, g->N, g->M, per_img, (size_t)per_img * g->M, 1, g->M, dtau_n, stream);
}

size_t cdl_fused2d_wgrad_workspace_floats(const cdl_geom *g)
{
    if (!fused_shape_ok(g)) return 0;
    // two regions of per-workgroup partials: a reverse sweep holds the stage's dA_k partials in the first and k_wgrad2d's
    // in the second until its one reduction launch per iteration; a stand-alone call uses the first.  k_wgrad2d's tiles
    // are 64 x 16 whatever the stage's shape, and only the 64 x 16 stage writes dA_k partials: one need for both shapes
    return 2 * wgrad_region_floats(g);
}

int cdl_fused2d_wgrad(const cdl_geom *g, const float *X0, const float *T0, float alpha0, float *dw0,
                      const float *X1, const float *T1, float alpha1, float *dw1, float *workspace,
                      int precision, void *stream)
{
    WgradReduce job;
    if (int rc = wgrad_partials(g, X0, T0, alpha0, dw0, X1, T1, alpha1, dw1, workspace, precision, stream, &job)) return rc;
    return launch_wgrad_reduce(g, job, S(stream));
}

int cdl_fused2d_assemble(const cdl_geom *g, const float *patches, const float *mask, const float *sub,
                         float alpha, float *out, float *acc, int acc_add, void *stream)
{
    return assemble<2>(g, patches, mask, sub, alpha, out, acc, acc_add, stream);
}

int cdl_fused2d_timing(int enable)
{
    std::lock_guard<std::mutex> lk(g_timing.mu);
    g_timing.on.store(enable != 0, std::memory_order_relaxed);
    if (enable) {
        for (auto &pr : g_timing.pairs) {
            g_timing.spare.push_back({pr.start, pr.dev});
            g_timing.spare.push_back({pr.stop, pr.dev});
        }
        g_timing.pairs.clear();
    }
    return 0;
}

int cdl_fused2d_timing_read(double *ms_sum, int *count)
{
    if (!ms_sum || !count) return CDL_EINVAL;
    std::lock_guard<std::mutex> lk(g_timing.mu);
    for (int c = 0; c < 4; ++c) { ms_sum[c] = 0.0; count[c] = 0; }
    for (auto &pr : g_timing.pairs) {
        float ms = 0.0f;
        hipError_t e = hipEventSynchronize(pr.stop);
        if (e == hipSuccess) e = hipEventElapsedTime(&ms, pr.start, pr.stop);
        if (e != hipSuccess) return -(int)e;
        ms_sum[pr.cls] += ms;
        ++count[pr.cls];
    }
    return 0;
}

int cdl_fused2d_forward(const cdl_geom *g, int K, const float *yp, const float *mask, const float *tau,
                        const float *const *wA, const float *const *wB, float *const *z, float *const *r,
                        unsigned *const *maps, float *xp, void *frags, float *patches, int precision,
                        const float *cmap, const float *tslope, void *stream)
{
    if (!fused_shape_ok(g)) return CDL_EUNSUPPORTED;
    if (K < 1 || !yp || !tau || !wA || !wB || !z || !xp || !frags || !patches || (K > 1 && !r)) return CDL_EINVAL;
    if (!cmap != !tslope) return CDL_EINVAL;
    const Flags f = parse_flags(precision);
    if (!f.ok || f.lout != 0) return CDL_EINVAL;
    if (f.lin == LAY_BLK16)                  // bf16 code storage: 64 x 32 tiles, two waves per SIMD (see the top of the file)
        return forward_sweep<4>(g, K, yp, mask, tau, wA, wB, z, r, maps, xp, frags, patches, f, stream, cmap, tslope);
    return forward_sweep<2>(g, K, yp, mask, tau, wA, wB, z, r, maps, xp, frags, patches, f, stream, cmap, tslope);
}

int cdl_fused2d_tangent(const cdl_geom *g, int K, const float *vp, const float *nvp, const float *mask,
                        const float *const *wA, const float *const *wB, const unsigned *const *maps, float *const *zd,
                        float *const *nrd, float *xdp, void *frags, float *patches, float *dtau_partial, int precision,
                        void *stream)
{
    if (!fused_shape_ok(g)) return CDL_EUNSUPPORTED;
    if (K < 1 || !vp || !nvp || !wA || !wB || !maps || !zd || !xdp || !frags || !patches || !dtau_partial || (K > 1 && !nrd))
        return CDL_EINVAL;
    const Flags f = parse_flags(precision);
    if (!f.ok || f.lout != 0) return CDL_EINVAL;
    if (f.lin == LAY_BLK16) return CDL_EUNSUPPORTED;          // tangent codes are fp32: no bf16 storage
    return tangent_sweep<2>(g, K, vp, nvp, mask, wA, wB, maps, zd, nrd, xdp, frags, patches, dtau_partial, f, stream);
}

int cdl_fused2d_backward(const cdl_geom *g, int K, const float *yp, const float *mask, const float *c,
                         const float *const *wA, const float *const *wB, const float *const *z,
                         const float *const *r, const unsigned *const *maps, const float *g_xp,
                         const float *g_z, float *const *dA,
                         float *const *dB, float *dt, float *du0, float *du1, float *q, void *frags,
                         float *patches, float *dtau_partial, float *wgrad_ws, int precision, float *dyp,
                         float *dtau, const float *cmap, const float *tslope, float *dcmap, void *stream)
{
    if (!fused_shape_ok(g)) return CDL_EUNSUPPORTED;
    if (K < 1 || !yp || !wA || !wB || !z || !maps || !g_xp || !dA || !dB || !dt || !du0 || !du1 || !q || !frags ||
        !patches || !dtau_partial || !wgrad_ws || (K > 1 && !r))
        return CDL_EINVAL;
    // a map: the thresholds' gradients are dt and dcmap -- no per-sample level c, no per-sample (K,N,M) dtau
    if (!cmap != !tslope || (dcmap && !cmap) || (cmap && (c || dtau))) return CDL_EINVAL;
    const Flags f = parse_flags(precision);
    if (!f.ok || f.lout != 0) return CDL_EINVAL;
    if (f.lin == LAY_BLK16)
        return backward_sweep<4>(g, K, yp, mask, c, wA, wB, z, r, maps, g_xp, g_z, dA, dB, dt, du0, du1, q, frags, patches,
                                 dtau_partial, wgrad_ws, f, dyp, dtau, stream, cmap, tslope, dcmap);
    return backward_sweep<2>(g, K, yp, mask, c, wA, wB, z, r, maps, g_xp, g_z, dA, dB, dt, du0, du1, q, frags, patches,
                             dtau_partial, wgrad_ws, f, dyp, dtau, stream, cmap, tslope, dcmap);
}

}  // extern "C"
