// Blind noise-level estimation by the median absolute deviation of the finest diagonal wavelet band
// (reference model/nle.py:17-27 nle_mad with model/wvlt.py:13-41):
//     HHy   = conv2d(y, hh, stride = 2, groups = C)      hh = flip(outer(dec_hi, dec_hi)) of 'bior4.4', 10 x 10
//     sigma = median(|HHy| over (C, H', W') per sample) / 0.6745          (torch.median: the LOWER median)
// Two kernels: the depthwise stride-2 correlation (the 2-D filter is an outer product, applied as such:
// 100 multiply-adds per output from registers) writing |HHy|, and an exact selection of the k-th smallest
// value per sample by a 3-pass radix histogram over the float bit patterns (non-negative floats order like
// their bits), integer counting only: the result is the bit-exact lower median of the band.
//
// The same two kernels serve the local estimates: the selection per cell of a grid over the band (cdl_nle_mad_cells,
// DESIGN.md section 19) and per bin of the local intensity (cdl_nle_nlf_bins, section 29: signal-dependent noise).
//
// The taps are PyWavelets' 'bior4.4' decomposition high-pass filter (pywt.Wavelet('bior4.4').dec_hi).  PyWavelets
// is not installed in the build image, so the table below is restated from the published CDF 9/7 pair; tests
// pin it through the perfect-reconstruction identity with the matching low-pass / reconstruction filters.
#include "cdl_common.h"

namespace {

constexpr int TAPS = 10;
constexpr int MEAN_FIRST = 2, MEAN_LAST = 8;               // the taps that are not zero: 7 x 7 pixels
// flip(dec_hi): conv2d correlates with the flipped outer product (wvlt.py:41 flips both axes)
__constant__ float c_hi_flipped[TAPS] = {0.0f,
                                         0.0f,
                                         -0.06453888262869706f,
                                         0.04068941760916406f,
                                         0.41809227322161724f,
                                         -0.7884856164055829f,
                                         0.41809227322161724f,
                                         0.04068941760916406f,
                                         -0.06453888262869706f,
                                         0.0f};

// one thread per output (n, c, i, j): |sum_a f[a] * (sum_b f[b] * y[2i + a][2j + b])|; with mean_out, also the mean of
// the 7 x 7 pixels under the non-zero taps (a, b = 2 .. 8), from the same loads: the local intensity the noise-level
// function bins by.  The chain that forms |HHy| is the same with and without it.
__global__ __launch_bounds__(256) void k_hh_abs(const float *__restrict__ y, float *__restrict__ out, int NC,
                                                int H, int W, int Ho, int Wo, float *__restrict__ mean_out)
{
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t total = (size_t)NC * Ho * Wo;
    if (idx >= total) return;
    const int j = (int)(idx % Wo);
    const size_t r = idx / Wo;
    const int i = (int)(r % Ho);
    const size_t nc = r / Ho;
    const float *base = y + (nc * H + 2 * i) * (size_t)W + 2 * j;
    float acc = 0.0f, sum = 0.0f;
#pragma unroll
    for (int a = 0; a < TAPS; ++a) {
        float row = 0.0f, rsum = 0.0f;
#pragma unroll
        for (int b = 0; b < TAPS; ++b) {
            const float v = base[(size_t)a * W + b];
            row = fmaf(c_hi_flipped[b], v, row);
            if (a >= MEAN_FIRST && a <= MEAN_LAST && b >= MEAN_FIRST && b <= MEAN_LAST) rsum += v;
        }
        acc = fmaf(c_hi_flipped[a], row, acc);
        if (a >= MEAN_FIRST && a <= MEAN_LAST) sum += rsum;
    }
    out[idx] = fabsf(acc);
    if (mean_out) mean_out[idx] = sum / (float)((MEAN_LAST - MEAN_FIRST + 1) * (MEAN_LAST - MEAN_FIRST + 1));
}

// k-th smallest (0-based) of `count` non-negative floats per sample: radix select, 11 + 11 + 10 bits.
__global__ __launch_bounds__(1024) void k_select(const float *__restrict__ v, float *__restrict__ out, size_t count,
                                                 size_t kth, float divisor)
{
    __shared__ unsigned hist[2048];
    __shared__ unsigned sel_prefix, sel_rank;
    const unsigned *bits = reinterpret_cast<const unsigned *>(v) + (size_t)blockIdx.x * count;
    unsigned prefix = 0, mask = 0;
    size_t rank = kth;                                     // rank of the target among the elements matching prefix
    const int shifts[3] = {21, 10, 0}, widths[3] = {11, 11, 10};
    for (int pass = 0; pass < 3; ++pass) {
        const int sh = shifts[pass], nb = 1 << widths[pass];
        for (int b = threadIdx.x; b < nb; b += blockDim.x) hist[b] = 0;
        __syncthreads();
        for (size_t e = threadIdx.x; e < count; e += blockDim.x) {
            const unsigned u = bits[e];
            if ((u & mask) == prefix) atomicAdd(&hist[(u >> sh) & (nb - 1)], 1u);
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            size_t seen = 0;
            int b = 0;
            for (; b < nb; ++b) {
                if (seen + hist[b] > rank) break;
                seen += hist[b];
            }
            sel_prefix = prefix | ((unsigned)b << sh);
            sel_rank = (unsigned)(rank - seen);
        }
        __syncthreads();
        prefix = sel_prefix;
        rank = sel_rank;
        mask |= (unsigned)(nb - 1) << sh;
        __syncthreads();
    }
    if (threadIdx.x == 0) out[blockIdx.x] = __builtin_bit_cast(float, prefix) / divisor;
}

// ---- local estimates: the same selection over a window of the band, one workgroup per (image, cell) ----
// Cells along an axis of band length L, window w, step q: one cell [0, L) if L <= w, otherwise ceil((L - w) / q) + 1
// cells of w samples, cell i starting at min(i * q, L - w) (the last one flush with the border).
__host__ __device__ inline int cell_count(int L, int w, int q) { return L <= w ? 1 : (L - w + q - 1) / q + 1; }
__host__ __device__ inline int cell_start(int i, int L, int w, int q) { return L <= w ? 0 : min(i * q, L - w); }

constexpr int CELL_THREADS = 256, CELL_WAVES = CELL_THREADS / 64;
// samples staged in LDS next to the 8 KB histogram: 56 KB a workgroup at the most, so two share a CU's 160 KB
constexpr int CELL_STAGE_MAX = 12288;

// k-th smallest of the C * ch * cw samples of one cell of the band (N, C, Hb, Wb), as k_select finds it (3 radix
// passes over the bit patterns, integer counting only), with the samples read once into LDS when STAGED (dynamic
// shared memory: 2048 histogram words, then the samples) and from the band in memory on every pass otherwise.  The
// bin holding the target rank is found by all threads: each sums nb / 256 consecutive bins, a wave-shuffle prefix
// scan orders the sums, and the one thread whose range holds the rank walks its own bins.
//
// Keyed mode (`key` non-null: the noise-level function): a workgroup is one (image, bin) pair,
// blockIdx.x = n * nbins + bin, its domain the whole band of the image, all channels, and its samples the members of
// the bin: those whose key m (the band of local means k_hh_abs wrote) has lo <= m < hi and
// (int)floorf((m - lo) * scale) == bin.  A counting pass ahead of the radix passes gives the number of members, hence
// the rank; STAGED, it also compacts the members into LDS (in any order: a selection does not depend on it), so the
// radix passes read no key; otherwise every pass reads both bands again, KEYED_LOADS samples a thread at a time so
// that the loads overlap (one workgroup scans a whole image: latency, not bandwidth, is what it waits for).  An empty
// bin writes 0, 0.
constexpr int KEYED_LOADS = 16;                            // loads a thread has in flight when the bins read the bands
constexpr float NO_KEY = __builtin_nanf("");               // the key of a sample past the end: a member of no bin

__device__ inline bool bin_member(float m, float lo, float hi, float scale, int bin)
{
    return m >= lo && m < hi && (int)floorf((m - lo) * scale) == bin;
}

template <bool STAGED>
__global__ __launch_bounds__(CELL_THREADS) void k_select_cells(const float *__restrict__ band,
                                                                float *__restrict__ out, int C, int Hb, int Wb, int w,
                                                                int q, int ny, int nx, float divisor,
                                                                const float *__restrict__ key, float lo, float hi,
                                                                float scale, int nbins, int *__restrict__ count_out)
{
    extern __shared__ unsigned cell_lds[];
    unsigned *hist = cell_lds, *stage = cell_lds + 2048;
    __shared__ unsigned wave_sum[CELL_WAVES], sel_prefix, sel_rank, members;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const bool keyed = key != nullptr;
    const int cx = blockIdx.x % nx, cy = (blockIdx.x / nx) % ny;
    const size_t n = keyed ? blockIdx.x / (unsigned)nbins : blockIdx.x / ((unsigned)nx * ny);
    const int bin = keyed ? (int)(blockIdx.x % (unsigned)nbins) : 0;
    const int ch = min(w, Hb), cw = min(w, Wb), y0 = cell_start(cy, Hb, w, q), x0 = cell_start(cx, Wb, w, q);
    const unsigned per_c = (unsigned)ch * cw;
    unsigned count = (unsigned)C * per_c;
    const unsigned domain = (unsigned)C * Hb * Wb;         // keyed: the candidates, contiguous from the image's first
    const unsigned *bits = reinterpret_cast<const unsigned *>(band) +
                           (keyed ? n * domain : (n * C * Hb + y0) * (size_t)Wb + x0);
    const float *keys = keyed ? key + n * domain : nullptr;
    auto load = [&](unsigned e) -> unsigned {              // sample e of the cell, (c, row, column) order
        const unsigned c = e / per_c, r = e % per_c;
        return bits[((size_t)c * Hb + r / cw) * Wb + r % cw];
    };
    if (keyed) {
        if (tid == 0) members = 0;
        __syncthreads();
        if (STAGED) {
            for (unsigned e0 = 0; e0 < domain; e0 += CELL_THREADS) {   // the same trip count for every lane of a wave
                const unsigned e = e0 + tid;
                const bool in = e < domain && bin_member(keys[e], lo, hi, scale, bin);
                const unsigned long long vote = __ballot(in);
                unsigned first = 0;                        // one LDS atomic per wave reserves the slots of its members
                if (lane == 0 && vote) first = atomicAdd(&members, (unsigned)__popcll(vote));
                first = __shfl(first, 0, 64);
                if (in) stage[first + __popcll(vote & ((1ull << lane) - 1))] = bits[e];
            }
        } else {
            unsigned mine = 0;
            for (unsigned e0 = tid; e0 < domain; e0 += CELL_THREADS * KEYED_LOADS) {
                float m[KEYED_LOADS];
#pragma unroll
                for (int u = 0; u < KEYED_LOADS; ++u) {
                    const unsigned e = e0 + u * CELL_THREADS;
                    m[u] = e < domain ? keys[e] : NO_KEY;
                }
#pragma unroll
                for (int u = 0; u < KEYED_LOADS; ++u) mine += bin_member(m[u], lo, hi, scale, bin) ? 1u : 0u;
            }
            if (mine) atomicAdd(&members, mine);
        }
        __syncthreads();
        count = members;
        if (tid == 0) {
            count_out[blockIdx.x] = (int)count;
            if (count == 0) out[blockIdx.x] = 0.0f;
        }
        if (count == 0) return;                            // the same for every thread: all leave here, after the barrier
    } else if (STAGED) {
        for (unsigned e = tid; e < count; e += CELL_THREADS) stage[e] = load(e);
    }
    unsigned prefix = 0, mask = 0, rank = (count - 1) / 2;  // torch.median: the lower of the two middle values
    const int shifts[3] = {21, 10, 0}, widths[3] = {11, 11, 10};
    for (int pass = 0; pass < 3; ++pass) {
        const int sh = shifts[pass], nb = 1 << widths[pass], per_t = nb / CELL_THREADS;
        for (int b = tid; b < nb; b += CELL_THREADS) hist[b] = 0;
        __syncthreads();
        if (keyed && !STAGED) {
            for (unsigned e0 = tid; e0 < domain; e0 += CELL_THREADS * KEYED_LOADS) {
                unsigned v[KEYED_LOADS];
                float m[KEYED_LOADS];
#pragma unroll
                for (int u = 0; u < KEYED_LOADS; ++u) {
                    const unsigned e = e0 + u * CELL_THREADS;
                    v[u] = e < domain ? bits[e] : 0u;
                    m[u] = e < domain ? keys[e] : NO_KEY;
                }
#pragma unroll
                for (int u = 0; u < KEYED_LOADS; ++u)
                    if ((v[u] & mask) == prefix && bin_member(m[u], lo, hi, scale, bin))
                        atomicAdd(&hist[(v[u] >> sh) & (nb - 1)], 1u);
            }
        } else {
            for (unsigned e = tid; e < count; e += CELL_THREADS) {
                const unsigned u = STAGED ? stage[e] : load(e);
                if ((u & mask) == prefix) atomicAdd(&hist[(u >> sh) & (nb - 1)], 1u);
            }
        }
        __syncthreads();
        unsigned mine = 0;
        for (int b = 0; b < per_t; ++b) mine += hist[tid * per_t + b];
        unsigned incl = mine;                                // inclusive scan over the wave, then over the 4 waves
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned up = __shfl_up(incl, d, 64);
            if (lane >= d) incl += up;
        }
        if (lane == 63) wave_sum[wave] = incl;
        __syncthreads();
        unsigned before = incl - mine;
        for (int v = 0; v < wave; ++v) before += wave_sum[v];
        if (before <= rank && rank < before + mine) {        // exactly one thread: the matching samples number > rank
            int b = tid * per_t;
            for (const int last = b + per_t - 1; b < last; ++b) {   // the rank is in this thread's bins: its last one if no earlier
                if (before + hist[b] > rank) break;
                before += hist[b];
            }
            sel_prefix = prefix | ((unsigned)b << sh);
            sel_rank = rank - before;
        }
        __syncthreads();
        prefix = sel_prefix;
        rank = sel_rank;
        mask |= (unsigned)(nb - 1) << sh;
    }
    if (tid == 0) out[blockIdx.x] = __builtin_bit_cast(float, prefix) / divisor;
}

}  // namespace

extern "C" {

size_t cdl_nle_mad_scratch_floats(int N, int C, int H, int W)
{
    if (N <= 0 || C <= 0 || H < TAPS || W < TAPS) return 0;
    return (size_t)N * C * ((H - TAPS) / 2 + 1) * ((W - TAPS) / 2 + 1);
}

int cdl_nle_mad(const float *y, float *sigma_hat, float *scratch, size_t scratch_floats, int N, int C, int H, int W,
                void *stream)
{
    if (!y || !sigma_hat || !scratch || N <= 0 || C <= 0) return CDL_EINVAL;
    if (H < TAPS || W < TAPS) return CDL_EINVAL;
    const int Ho = (H - TAPS) / 2 + 1, Wo = (W - TAPS) / 2 + 1;
    const size_t total = (size_t)N * C * Ho * Wo, per_n = (size_t)C * Ho * Wo;
    if (scratch_floats < total) return CDL_EINVAL;
    k_hh_abs<<<(unsigned)((total + 255) / 256), 256, 0, S(stream)>>>(y, scratch, N * C, H, W, Ho, Wo, nullptr);
    CDL_LAUNCH_CHECK();
    // torch.median returns the lower of the two middle values: 0-based rank (n - 1) / 2
    k_select<<<(unsigned)N, 1024, 0, S(stream)>>>(scratch, sigma_hat, per_n, (per_n - 1) / 2, 0.6745f);
    CDL_LAUNCH_CHECK();
    return 0;
}

size_t cdl_nle_mad_cells_scratch_floats(int N, int C, int H, int W)
{
    return cdl_nle_mad_scratch_floats(N, C, H, W);
}

// The bins of a keyed selection; bins == 0: cells, no key.
struct nlf_bins {
    int bins;
    float lo, hi, scale;
    int *count;
};

// The band of y into `band` (and its local means into `key`, for a keyed selection), then one selection per workgroup:
// per cell of the (window, step) grid, or per (image, bin) with `nb.bins` > 0.  `count`: the samples a workgroup may
// have to hold, which decides whether they are staged in LDS.  Arguments are checked by the callers.
static int band_and_select(const float *y, float *out, float *band, float *key, int N, int C, int H, int W, int window,
                           int step, const nlf_bins &nb, void *stream)
{
    const int Ho = (H - TAPS) / 2 + 1, Wo = (W - TAPS) / 2 + 1;
    const size_t total = (size_t)N * C * Ho * Wo;
    const int ny = nb.bins ? 1 : cell_count(Ho, window, step), nx = nb.bins ? 1 : cell_count(Wo, window, step);
    const size_t blocks = nb.bins ? (size_t)N * nb.bins : (size_t)N * ny * nx;
    const size_t count = nb.bins ? (size_t)C * Ho * Wo : (size_t)C * min(window, Ho) * min(window, Wo);
    if (blocks > 0x7fffffffu || count > 0x7fffffffu) return CDL_EINVAL;
    k_hh_abs<<<(unsigned)((total + 255) / 256), 256, 0, S(stream)>>>(y, band, N * C, H, W, Ho, Wo, key);
    CDL_LAUNCH_CHECK();
    CDL_TRACE_NOTE("k_select_cells<%s>%s", count <= (size_t)CELL_STAGE_MAX ? "true" : "false", nb.bins ? " keyed" : "");
    if (count <= (size_t)CELL_STAGE_MAX)
        k_select_cells<true><<<(unsigned)blocks, CELL_THREADS, (2048 + count) * sizeof(unsigned), S(stream)>>>(
            band, out, C, Ho, Wo, window, step, ny, nx, 0.6745f, key, nb.lo, nb.hi, nb.scale, nb.bins, nb.count);
    else
        k_select_cells<false><<<(unsigned)blocks, CELL_THREADS, 2048 * sizeof(unsigned), S(stream)>>>(
            band, out, C, Ho, Wo, window, step, ny, nx, 0.6745f, key, nb.lo, nb.hi, nb.scale, nb.bins, nb.count);
    CDL_LAUNCH_CHECK();
    return 0;
}

int cdl_nle_mad_cells(const float *y, float *cells, float *scratch, size_t scratch_floats, int N, int C, int H, int W,
                      int window, int step, void *stream)
{
    if (!y || !cells || !scratch || N <= 0 || C <= 0) return CDL_EINVAL;
    if (H < TAPS || W < TAPS || window < 2 || step < 1) return CDL_EINVAL;
    if (scratch_floats < cdl_nle_mad_scratch_floats(N, C, H, W)) return CDL_EINVAL;
    return band_and_select(y, cells, scratch, nullptr, N, C, H, W, window, step, nlf_bins{0, 0.0f, 0.0f, 0.0f, nullptr},
                           stream);
}

size_t cdl_nle_nlf_bins_scratch_floats(int N, int C, int H, int W)
{
    return 2 * cdl_nle_mad_scratch_floats(N, C, H, W);
}

int cdl_nle_nlf_bins(const float *y, float *sigma_bins, int *count_bins, float *scratch, size_t scratch_floats, int N,
                     int C, int H, int W, int bins, float lo, float hi, void *stream)
{
    if (!y || !sigma_bins || !count_bins || !scratch || N <= 0 || C <= 0) return CDL_EINVAL;
    if (H < TAPS || W < TAPS || bins < 1 || !(hi > lo)) return CDL_EINVAL;
    const size_t band = cdl_nle_mad_scratch_floats(N, C, H, W);
    if (scratch_floats < 2 * band) return CDL_EINVAL;
    const float scale = (float)((double)bins / ((double)hi - (double)lo));     // rounded to fp32 once, here
    if (!(scale > 0.0f) || !(scale <= 3.0e38f)) return CDL_EINVAL;             // a range too narrow for fp32 bins
    return band_and_select(y, sigma_bins, scratch, scratch + band, N, C, H, W, 2, 1, nlf_bins{bins, lo, hi, scale, count_bins},
                           stream);
}

}  // extern "C"
