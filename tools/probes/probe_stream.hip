// GPU-box diagnostic: what a pure load -> store stream reaches on MI355X with the ACCESS SHAPES of the fused
// iteration kernel (cdl_fused2d.hip), so that the kernel's 4.5-5.2 TB/s can be judged against a ceiling
// measured on the same box rather than against torch's copy_.  Shapes (all move 2 x 1.07 GB = cfg2's code tensor):
//   copy16      : grid-stride float4 copy, 2048 x 256 threads (the guide's 6.29 TB/s reference)
//   plane       : persistent 512-thread workgroups, 64 x 32 pixel tiles, per 32-pixel row block of a wave 32
//                 dword buffer loads whose addresses are one channel plane (H*W*4 B = 256 KiB) apart, then 32
//                 dword stores of the same shape -- k_stage's fat accesses as they stand
//   plane_pad   : the same with the channel planes 256 B further apart (stride H*W + 64 floats)
//   blocked16   : the same tile walk on a pixel-blocked layout [n][y][x/32][M/4][32 px][4 ch]: a lane's 4
//                 consecutive channels are 16 B, a wave instruction covers 1 KiB contiguous, a row block
//                 8 KiB contiguous (8 dwordx4 loads + 8 dwordx4 stores)
//   blocked8    : blocked layout with bf16 storage (4 channels = 8 B per lane; half the bytes)
// PF = 1 variants issue the next row block's loads before storing the current one (two blocks in flight).
// Output: one JSON line per variant with GB/s (median of REPS launches).
#include <hip/hip_runtime.h>
#include <type_traits>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e_), __LINE__); exit(1); } } while (0)

constexpr int N = 64, M = 64, H = 256, W = 256;
constexpr int TW = 64, TH = 32, RB = 8;
constexpr int OOB = 0x7fff0000;
typedef __attribute__((ext_vector_type(4))) unsigned u32x4;
typedef __attribute__((ext_vector_type(2))) unsigned u32x2;

__global__ __launch_bounds__(256) void k_copy16(const float4 *__restrict__ in, float4 *__restrict__ out, size_t n4)
{
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) out[i] = in[i];
}

__device__ __forceinline__ __amdgpu_buffer_rsrc_t rsrc(const void *base, size_t bytes)
{
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(base), 0, (int)bytes, 0x00020000);
}

// k_stage's shape: lane (c, h) of wave (wxi, wyi) owns pixel column wxi*32 + c; register v of tile R is
// channel 32R + 8(v>>2) + 4h + (v&3)
template <int PF>
__global__ __launch_bounds__(512) void k_plane(const float *__restrict__ in, float *__restrict__ out, int plane /*floats*/)
{
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wxi = wid % 2, wyi = wid / 2, c = lane & 31, h = lane >> 5;
    const int tilesX = W / TW, tilesY = H / TH, numTiles = N * tilesX * tilesY;
    const size_t img = (size_t)M * plane;
    const int hw4 = plane * 4;
    for (int t = blockIdx.x; t < numTiles; t += gridDim.x) {
        int bid = t;
        const int txi = bid % tilesX; bid /= tilesX;
        const int tyi = bid % tilesY;
        const int n = bid / tilesY;
        const int x = txi * TW + wxi * 32 + c;
        const __amdgpu_buffer_rsrc_t ri = rsrc(in + (size_t)n * img, img * 4), ro = rsrc(out + (size_t)n * img, img * 4);
        const int lane_off = (4 * h * plane + x) * 4;
        float zc[2][32];
        auto load = [&](int b, float (&dst)[32]) {
            const int y = tyi * TH + wyi * RB + b;
            const int voff = lane_off + y * W * 4;
#pragma unroll
            for (int i = 0; i < 32; ++i) {
                const int R = i >> 4, v = i & 15;
                dst[i] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(ri, voff, (32 * R + 8 * (v >> 2) + (v & 3)) * hw4, 0));
            }
        };
        auto store = [&](int b, const float (&src)[32]) {
            const int y = tyi * TH + wyi * RB + b;
            const int voff = lane_off + y * W * 4;
#pragma unroll
            for (int i = 0; i < 32; ++i) {
                const int R = i >> 4, v = i & 15;
                __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, src[i] + 1.0f), ro, voff, (32 * R + 8 * (v >> 2) + (v & 3)) * hw4, 0);
            }
        };
        if (PF == 0) {
#pragma unroll 1
            for (int b = 0; b < RB; ++b) { load(b, zc[0]); store(b, zc[0]); }
        } else {
            load(0, zc[0]);
#pragma unroll 1
            for (int b = 0; b < RB; b += 2) {
                load(b + 1, zc[1]);
                store(b, zc[0]);
                if (b + 2 < RB) load(b + 2, zc[0]);
                store(b + 1, zc[1]);
            }
        }
    }
}

// blocked layout: [n][y][xb][q = M/4][32 px][4 ch]; EB = bytes per lane access (16: fp32, 8: bf16)
template <int PF, int EB>
__global__ __launch_bounds__(512) void k_blocked(const char *__restrict__ in, char *__restrict__ out)
{
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wxi = wid % 2, wyi = wid / 2, c = lane & 31, h = lane >> 5;
    const int tilesX = W / TW, tilesY = H / TH, numTiles = N * tilesX * tilesY;
    constexpr int XB = W / 32, Q = M / 4;
    constexpr size_t rowblk = (size_t)Q * 32 * EB;              // bytes of one (y, xb) block: 8 KiB fp32
    const size_t img = (size_t)H * XB * rowblk;
    typedef typename std::conditional<EB == 16, u32x4, u32x2>::type vec;
    for (int t = blockIdx.x; t < numTiles; t += gridDim.x) {
        int bid = t;
        const int txi = bid % tilesX; bid /= tilesX;
        const int tyi = bid % tilesY;
        const int n = bid / tilesY;
        const int xb = txi * 2 + wxi;
        const __amdgpu_buffer_rsrc_t ri = rsrc(in + (size_t)n * img, img), ro = rsrc(out + (size_t)n * img, img);
        vec zc[2][8];
        auto load = [&](int b, vec (&dst)[8]) {
            const int y = tyi * TH + wyi * RB + b;
            const int voff = (int)(((size_t)y * XB + xb) * rowblk) + (h * 32 + c) * EB;
#pragma unroll
            for (int i = 0; i < 8; ++i) {                       // quad 2i + h: R = i >> 2, v>>2 = i & 3
                if constexpr (EB == 16) dst[i] = __builtin_bit_cast(vec, __builtin_amdgcn_raw_buffer_load_b128(ri, voff, i * 2 * 32 * EB, 0));
                else dst[i] = __builtin_bit_cast(vec, __builtin_amdgcn_raw_buffer_load_b64(ri, voff, i * 2 * 32 * EB, 0));
            }
        };
        auto store = [&](int b, vec (&src)[8]) {
            const int y = tyi * TH + wyi * RB + b;
            const int voff = (int)(((size_t)y * XB + xb) * rowblk) + (h * 32 + c) * EB;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                vec v = src[i];
                v.x += 1u;
                if constexpr (EB == 16) __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), ro, voff, i * 2 * 32 * EB, 0);
                else __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, v), ro, voff, i * 2 * 32 * EB, 0);
            }
        };
        if (PF == 0) {
#pragma unroll 1
            for (int b = 0; b < RB; ++b) { load(b, zc[0]); store(b, zc[0]); }
        } else {
            load(0, zc[0]);
#pragma unroll 1
            for (int b = 0; b < RB; b += 2) {
                load(b + 1, zc[1]);
                store(b, zc[0]);
                if (b + 2 < RB) load(b + 2, zc[0]);
                store(b + 1, zc[1]);
            }
        }
    }
}

typedef __attribute__((ext_vector_type(4))) float f32x4;
// ---- read-only / write-only / copy streams over 256 MB .. 4 GB, default and non-temporal cache policy -----------
// (the f32x4 copy reaches 5.07 TB/s on this pool's boxes where the guide quotes 6.29; is a
// read-only kernel such as k_wgrad2d under the same ceiling?)  Each thread keeps U independent 16-byte accesses in
// flight per trip; grid-stride over the buffer.
template <int U, bool NT>
__global__ __launch_bounds__(256) void k_read(const f32x4 *__restrict__ in, float *__restrict__ sink, size_t n4)
{
    float acc = 0.0f;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (; i + (U - 1) * stride < n4; i += U * stride) {
        f32x4 v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) v[u] = NT ? __builtin_nontemporal_load(&in[i + u * stride]) : in[i + u * stride];
#pragma unroll
        for (int u = 0; u < U; ++u) acc += v[u].x + v[u].y + v[u].z + v[u].w;
    }
    for (; i < n4; i += stride) { const f32x4 v = in[i]; acc += v.x + v.y + v.z + v.w; }
    if (acc == 123.456f) sink[threadIdx.x] = acc;              // never true for the fill pattern: keeps the loads alive
}

template <int U, bool NT>
__global__ __launch_bounds__(256) void k_write(f32x4 *__restrict__ out, size_t n4, float val)
{
    const f32x4 v = f32x4{val, val + 1.0f, val + 2.0f, val + 3.0f};
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (; i + (U - 1) * stride < n4; i += U * stride) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (NT) __builtin_nontemporal_store(v, &out[i + u * stride]);
            else out[i + u * stride] = v;
        }
    }
    for (; i < n4; i += stride) out[i] = v;
}

template <int U, bool NT>
__global__ __launch_bounds__(256) void k_copy(const f32x4 *__restrict__ in, f32x4 *__restrict__ out, size_t n4)
{
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (; i + (U - 1) * stride < n4; i += U * stride) {
        f32x4 v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) v[u] = NT ? __builtin_nontemporal_load(&in[i + u * stride]) : in[i + u * stride];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (NT) __builtin_nontemporal_store(v[u], &out[i + u * stride]);
            else out[i + u * stride] = v[u];
        }
    }
    for (; i < n4; i += stride) out[i] = in[i];
}

template <class F>
static double time_ms(F launch, int reps)
{
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    for (int i = 0; i < 3; ++i) launch();
    std::vector<float> ms(reps);
    for (int i = 0; i < reps; ++i) {
        CK(hipEventRecord(e0, 0));
        launch();
        CK(hipEventRecord(e1, 0));
        CK(hipEventSynchronize(e1));
        CK(hipEventElapsedTime(&ms[i], e0, e1));
    }
    CK(hipGetLastError());
    std::sort(ms.begin(), ms.end());
    return ms[reps / 2];
}

static void rw_probes(int reps)
{
    const size_t maxb = (size_t)4 << 30;
    f32x4 *a, *b;
    float *sink;
    CK(hipMalloc(&a, maxb)); CK(hipMalloc(&b, maxb)); CK(hipMalloc(&sink, 4096));
    CK(hipMemset(a, 0x3c, maxb)); CK(hipMemset(b, 0, maxb));
    auto report = [&](const char *kind, const char *policy, int U, int grid, size_t bytes_buf, double ms, double moved) {
        printf("{\"probe\": \"%s\", \"policy\": \"%s\", \"loads_in_flight\": %d, \"grid\": %d, \"buffer_MB\": %zu, "
               "\"ms\": %.4f, \"GBps\": %.1f, \"frac_of_8TBps\": %.3f}\n", kind, policy, U, grid, bytes_buf >> 20, ms,
               moved / ms * 1e-6, moved / ms * 1e-6 / 8000.0);
        fflush(stdout);
    };
    for (size_t bytes : {(size_t)256 << 20, (size_t)1 << 30, (size_t)2 << 30, (size_t)4 << 30}) {
        const size_t n4 = bytes / 16;
        for (int grid : {2048, 8192}) {
            report("read-only", "default", 1, grid, bytes, time_ms([&] { k_read<1, false><<<grid, 256>>>(a, sink, n4); }, reps), (double)bytes);
            report("read-only", "default", 4, grid, bytes, time_ms([&] { k_read<4, false><<<grid, 256>>>(a, sink, n4); }, reps), (double)bytes);
            report("read-only", "nt", 4, grid, bytes, time_ms([&] { k_read<4, true><<<grid, 256>>>(a, sink, n4); }, reps), (double)bytes);
            report("write-only", "default", 1, grid, bytes, time_ms([&] { k_write<1, false><<<grid, 256>>>(b, n4, 1.0f); }, reps), (double)bytes);
            report("write-only", "default", 4, grid, bytes, time_ms([&] { k_write<4, false><<<grid, 256>>>(b, n4, 1.0f); }, reps), (double)bytes);
            report("write-only", "nt", 4, grid, bytes, time_ms([&] { k_write<4, true><<<grid, 256>>>(b, n4, 1.0f); }, reps), (double)bytes);
            report("copy", "default", 1, grid, bytes, time_ms([&] { k_copy<1, false><<<grid, 256>>>(a, b, n4); }, reps), 2.0 * bytes);
            report("copy", "default", 4, grid, bytes, time_ms([&] { k_copy<4, false><<<grid, 256>>>(a, b, n4); }, reps), 2.0 * bytes);
            report("copy", "nt", 4, grid, bytes, time_ms([&] { k_copy<4, true><<<grid, 256>>>(a, b, n4); }, reps), 2.0 * bytes);
        }
    }
    CK(hipFree(a)); CK(hipFree(b)); CK(hipFree(sink));
}

// ---- cache policy per stream (./probe_stream REPS policy) ------------------------------------------------------------
// The aux immediate of the buffer builtins on gfx950: 0 plain, 1 sc0, 2 nt, 16 sc1 (stores: write-through; loads: past
// the CU's L1), 17 sc0 sc1, 18 nt sc1.  Nothing but buffer loads and stores carries a policy here.
//   stage64x16 : k_stage's fat streams as the flagship runs them -- 4 waves, 64 x 16 tiles with stride gridDim.x from the
//                first tile (rev 0) or the last (rev 1), blocked layout, 8 x 16 B per lane and row block; the forms are
//                read-only, write-only and copy (copy ping-pongs between the two tensors and alternates rev from launch
//                to launch, as the stages of a sweep do)
//   wgrad64x16 : k_wgrad2d's fat load -- 8 waves, the two wave groups on alternate tiles, loads one row block ahead
//   boundary   : a kernel that leaves 30 MB behind as patch-like 16-byte stores (6160-byte runs per tile, every
//                workgroup) and a dependent kernel that reads them back
// The variants are interleaved: one launch of each per round, REPS rounds per direction; median and min per variant.
constexpr int POL[6] = {0, 1, 2, 16, 17, 18};
enum { F_READ = 0, F_WRITE = 1, F_COPY = 2 };
constexpr int PTH = 16, PXB = W / 32, PQ = M / 4;
constexpr int PROWBLK = PQ * 32 * 16;                          // 8 KiB: one (y, xb) block
constexpr size_t PIMG = (size_t)H * PXB * PROWBLK;             // 16 MiB per image: every offset fits the descriptor
constexpr int PTILES = N * (W / TW) * (H / PTH);

template <int FORM, int LD, int ST>
__global__ __launch_bounds__(256) void k_pol_stage(const char *__restrict__ in, char *__restrict__ out, float *__restrict__ sink, int rev)
{
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wxi = wid % 2, wyi = wid / 2, c = lane & 31, h = lane >> 5;
    constexpr int tilesX = W / TW, tilesY = H / PTH;
    unsigned acc = 0;
    for (int t = blockIdx.x; t < PTILES; t += gridDim.x) {
        int bid = rev ? PTILES - 1 - t : t;
        const int txi = bid % tilesX; bid /= tilesX;
        const int tyi = bid % tilesY;
        const int n = bid / tilesY;
        const int xb = txi * 2 + wxi;
        const __amdgpu_buffer_rsrc_t ri = rsrc(in + (size_t)n * PIMG, PIMG), ro = rsrc(out + (size_t)n * PIMG, PIMG);
#pragma unroll 1
        for (int b = 0; b < RB; ++b) {
            const int y = tyi * PTH + wyi * RB + b;
            const int voff = (y * PXB + xb) * PROWBLK + (h * 32 + c) * 16;
            u32x4 v[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                if (FORM != F_WRITE) v[i] = __builtin_amdgcn_raw_buffer_load_b128(ri, voff, i * 2 * 32 * 16, LD);
                else v[i] = u32x4{(unsigned)t, (unsigned)b, (unsigned)i, (unsigned)rev};
            }
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                if (FORM == F_READ) { acc += v[i].x ^ v[i].y ^ v[i].z ^ v[i].w; continue; }
                v[i].x += 1u;
                // a store of more than 8 bytes keeps its scalar offset an immediate (cdl_fused2d.hip, blk_store4)
                __builtin_amdgcn_raw_buffer_store_b128(v[i], ro, voff + i * 2 * 32 * 16, 0, ST);
            }
        }
    }
    if (FORM == F_READ && acc == 0x12345678u) sink[tid] = 1.0f;     // keeps the loads alive
}

template <int LD>
__global__ __launch_bounds__(512) void k_pol_wgrad(const char *__restrict__ in, char *__restrict__, float *__restrict__ sink, int rev)
{
    const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int op = wid >> 2, wq = wid & 3, wxi = wq & 1, wyi = wq >> 1, c = lane & 31, h = lane >> 5;
    constexpr int tilesX = W / TW, tilesY = H / PTH, nsteps = (PTILES + 1) / 2;
    unsigned acc = 0;
    auto load = [&](u32x4 (&v)[8], int t0, int b) {
        const int t = 2 * t0 + op;
        const bool active = t0 < nsteps && t < PTILES;
        int bid = rev ? PTILES - 1 - t : t;
        const int txi = bid % tilesX; bid /= tilesX;
        const int tyi = bid % tilesY;
        const int n = active ? bid / tilesY : 0;
        const int y = tyi * PTH + wyi * RB + b, xb = txi * 2 + wxi;
        const __amdgpu_buffer_rsrc_t ri = rsrc(in + (size_t)n * PIMG, PIMG);
        const int voff = active ? (y * PXB + xb) * PROWBLK + (h * 32 + c) * 16 : OOB;
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = __builtin_amdgcn_raw_buffer_load_b128(ri, voff, i * 2 * 32 * 16, LD);
    };
    auto use = [&](const u32x4 (&v)[8]) {
#pragma unroll
        for (int i = 0; i < 8; ++i) acc += v[i].x ^ v[i].y ^ v[i].z ^ v[i].w;
    };
    u32x4 va[8], vb[8];
    load(va, blockIdx.x, 0);
    for (int t0 = blockIdx.x; t0 < nsteps; t0 += gridDim.x) {
#pragma unroll 1
        for (int b = 0; b < RB; b += 2) {
            load(vb, t0, b + 1);
            use(va);
            if (b + 2 < RB) load(va, t0, b + 2); else load(va, t0 + gridDim.x, 0);
            use(vb);
        }
    }
    if (acc == 0x12345678u) sink[tid] = 1.0f;
}

constexpr int BCHUNK = 385;                                    // 16-byte vectors of one 22 x 70 patch (6160 B)
constexpr int BTILES = 4870;                                   // x 6160 B = 30.0 MB
template <int ST>
__global__ __launch_bounds__(256) void k_bnd_write(const char *__restrict__, char *__restrict__ out, float *__restrict__, int rev)
{
    const __amdgpu_buffer_rsrc_t ro = rsrc(out, (size_t)BTILES * BCHUNK * 16);
    for (int t = blockIdx.x; t < BTILES; t += gridDim.x)
        for (int i = threadIdx.x; i < BCHUNK; i += 256)
            __builtin_amdgcn_raw_buffer_store_b128(u32x4{(unsigned)t, (unsigned)i, (unsigned)rev, 1u}, ro, (t * BCHUNK + i) * 16, 0, ST);
}
__global__ __launch_bounds__(256) void k_bnd_read(const char *__restrict__ in, char *__restrict__, float *__restrict__ sink, int)
{
    const u32x4 *src = reinterpret_cast<const u32x4 *>(in);
    const size_t n = (size_t)BTILES * BCHUNK;
    unsigned acc = 0;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const u32x4 v = src[i];
        acc += v.x ^ v.y ^ v.z ^ v.w;
    }
    if (acc == 0x12345678u) sink[threadIdx.x] = 1.0f;
}

typedef void (*pol_kernel)(const char *, char *, float *, int);
struct Variant {
    const char *shape, *form;
    int ld, st, block;
    pol_kernel k, k2;                    // k2: the dependent reader of the boundary pair (nullptr elsewhere)
    double bytes;
    std::vector<float> ms[2];            // per direction
};
template <int LI = 0, int SI = 0>
static void add_copies(std::vector<Variant> &v, double bytes)
{
    if constexpr (LI < 6) {
        v.push_back({"stage64x16", "copy", POL[LI], POL[SI], 256, k_pol_stage<F_COPY, POL[LI], POL[SI]>, nullptr, 2 * bytes, {}});
        if constexpr (SI + 1 < 6) add_copies<LI, SI + 1>(v, bytes); else add_copies<LI + 1, 0>(v, bytes);
    }
}
template <int I = 0>
static void add_singles(std::vector<Variant> &v, double bytes)
{
    if constexpr (I < 6) {
        v.push_back({"stage64x16", "read-only", POL[I], -1, 256, k_pol_stage<F_READ, POL[I], 0>, nullptr, bytes, {}});
        v.push_back({"stage64x16", "write-only", -1, POL[I], 256, k_pol_stage<F_WRITE, 0, POL[I]>, nullptr, bytes, {}});
        v.push_back({"wgrad64x16", "read-only", POL[I], -1, 512, k_pol_wgrad<POL[I]>, nullptr, bytes, {}});
        const double bb = (double)BTILES * BCHUNK * 16;
        v.push_back({"boundary", "write-30MB", -1, POL[I], 256, k_bnd_write<POL[I]>, nullptr, bb, {}});
        v.push_back({"boundary", "write-30MB+dependent-read", -1, POL[I], 256, k_bnd_write<POL[I]>, k_bnd_read, 2 * bb, {}});
        add_singles<I + 1>(v, bytes);
    }
}

static void policy_probes(int reps)
{
    char *a, *b;
    float *sink;
    const size_t bytes = (size_t)N * PIMG;
    CK(hipMalloc(&a, bytes)); CK(hipMalloc(&b, bytes)); CK(hipMalloc(&sink, 4096));
    CK(hipMemset(a, 0x3c, bytes)); CK(hipMemset(b, 0, bytes));
    std::vector<Variant> vs;
    add_singles(vs, (double)bytes);
    add_copies(vs, (double)bytes);
    vs.push_back({"boundary", "dependent-read-alone", 0, -1, 256, k_bnd_read, nullptr, (double)BTILES * BCHUNK * 16, {}});
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    const int grid = 256;
    for (int r = -2; r < 2 * reps; ++r) {                      // two warm-up rounds
        const int rev = r & 1;
        for (Variant &v : vs) {
            const char *src = rev ? b : a;                     // ping-pong, as z_k / z_{k+1} do
            char *dst = rev ? a : b;
            CK(hipEventRecord(e0, 0));
            v.k<<<grid, v.block>>>(src, dst, sink, rev);
            if (v.k2) v.k2<<<grid, v.block>>>(dst, nullptr, sink, rev);
            CK(hipEventRecord(e1, 0));
            CK(hipEventSynchronize(e1));
            float ms;
            CK(hipEventElapsedTime(&ms, e0, e1));
            if (r >= 0) v.ms[rev].push_back(ms);
        }
    }
    CK(hipGetLastError());
    for (Variant &v : vs)
        for (int rev = 0; rev < 2; ++rev) {
            std::vector<float> &m = v.ms[rev];
            std::sort(m.begin(), m.end());
            const double med = m[m.size() / 2], mn = m[0];
            printf("{\"probe\": \"cache-policy\", \"shape\": \"%s\", \"form\": \"%s\", \"ld_aux\": %d, \"st_aux\": %d, \"rev\": %d, "
                   "\"launches\": %zu, \"median_ms\": %.4f, \"min_ms\": %.4f, \"median_GBps\": %.1f, \"best_GBps\": %.1f}\n",
                   v.shape, v.form, v.ld, v.st, rev, m.size(), med, mn, v.bytes / med * 1e-6, v.bytes / mn * 1e-6);
        }
    CK(hipFree(a)); CK(hipFree(b)); CK(hipFree(sink));
}

int main(int argc, char **argv)
{
    const int reps = argc > 1 ? atoi(argv[1]) : 15;
    if (argc > 2 && argv[2][0] == 'r') { rw_probes(reps); return 0; }     // ./probe_stream 15 rw
    if (argc > 2 && argv[2][0] == 'p') { policy_probes(reps); return 0; } // ./probe_stream 15 policy
    const size_t floats = (size_t)N * M * (H * W + 64);         // room for the padded planes
    float *in, *out;
    CK(hipMalloc(&in, floats * 4)); CK(hipMalloc(&out, floats * 4));
    CK(hipMemset(in, 0x3c, floats * 4)); CK(hipMemset(out, 0, floats * 4));
    const double bytes = 2.0 * N * M * H * W * 4;
    int cus = 256;
    CK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, 0));
    auto report = [&](const char *name, int grid, double ms, double b) {
        printf("{\"probe\": \"%s\", \"grid\": %d, \"ms\": %.4f, \"GBps\": %.1f, \"frac_of_8TBps\": %.3f}\n", name, grid, ms, b / ms * 1e-6,
               b / ms * 1e-6 / 8000.0);
        fflush(stdout);
    };
    const size_t n4 = (size_t)N * M * H * W / 4;
    for (int g : {2048, 8192})
        report("copy16 (float4 grid-stride, 256 threads)", g,
               time_ms([&] { k_copy16<<<g, 256>>>((const float4 *)in, (float4 *)out, n4); }, reps), bytes);
    for (int g : {cus, 2 * cus}) {
        report("plane dword, stride H*W (k_stage today)", g, time_ms([&] { k_plane<0><<<g, 512>>>(in, out, H * W); }, reps), bytes);
        report("plane dword, stride H*W, 2 row blocks in flight", g, time_ms([&] { k_plane<1><<<g, 512>>>(in, out, H * W); }, reps), bytes);
        report("plane dword, stride H*W+64", g, time_ms([&] { k_plane<0><<<g, 512>>>(in, out, H * W + 64); }, reps), bytes);
        report("plane dword, stride H*W+64, 2 row blocks in flight", g, time_ms([&] { k_plane<1><<<g, 512>>>(in, out, H * W + 64); }, reps), bytes);
        report("blocked 16 B (1 KiB per instruction)", g, time_ms([&] { k_blocked<0, 16><<<g, 512>>>((const char *)in, (char *)out); }, reps), bytes);
        report("blocked 16 B, 2 row blocks in flight", g, time_ms([&] { k_blocked<1, 16><<<g, 512>>>((const char *)in, (char *)out); }, reps), bytes);
        report("blocked 8 B (bf16 storage)", g, time_ms([&] { k_blocked<0, 8><<<g, 512>>>((const char *)in, (char *)out); }, reps), bytes / 2);
        report("blocked 8 B (bf16 storage), 2 row blocks in flight", g, time_ms([&] { k_blocked<1, 8><<<g, 512>>>((const char *)in, (char *)out); }, reps), bytes / 2);
    }
    return 0;
}
