// The perceptual term of the reference's CombinedLossWithSSIM (loss.py): VGG16 features[:16] (relu3_3) of every frame of
// `output` and `target`, the mean squared difference of the two feature maps, and its gradient with respect to either
// image.  A call covers P independent one-channel H x W planes (a (B, 1, T, H, W) clip is B*T planes, no copy).
//
// Forward, per image (target first, then output):
//     conv1_1  1 -> 64 at (H, W)            k_vgg_conv11 (the three identical input channels: weights summed over them)
//     conv1_2  64 -> 64, max-pool           dense tier, CDL_VGG_POOL  -> (H2, W2) = floor(H/2, W/2) + argmax codes
//     conv2_1  64 -> 128                    dense tier, CDL_VGG_BIAS
//     conv2_2  128 -> 128, max-pool         dense tier, CDL_VGG_POOL  -> (H4, W4) + argmax codes
//     conv3_1, conv3_2  -> 256              dense tier, CDL_VGG_BIAS
//     conv3_3  256 -> 256                   target: CDL_VGG_BIAS (fy = relu3_3); output: CDL_VGG_DIFF
// every convolution 3x3, padding 1, bias, ReLU.  CDL_VGG_DIFF writes the backward's seeds d [fx > 0], d [fy > 0]
// (d = fx - fy) and one fp64 sum of d^2 per workgroup, which k_vgg_fold adds in a fixed order: loss = sum / n,
// n = P * 256 * H4 * W4.
//
// Backward, per requested image: the transposed layers on the dense tier's synthesis role, each ReLU a gate on the
// kept activations (out_gate), the pooled layers' gate the pooled activation (its window's maximum); the unpool is a
// staging mode of the next transposed convolution (CDL_VGG_UNPOOL), so no full-resolution gradient is written before
// it is consumed.  The 64 -> 1 transposed conv1_1 is cdl_synthesis gated by relu1_1.  The map is linear in the seed:
// k_vgg_scale applies 2/n times the upstream gradient (a device scalar; -2/n for the target) once, at the end.
// No atomics: repeated calls are bit-identical.
#include "cdl_common.h"

namespace {

constexpr int CX = 64, CY = 4;                 // k_vgg_conv11 tile: 64 columns x 4 rows, one thread per pixel

__global__ __launch_bounds__(CX * CY) void k_vgg_conv11(const float *__restrict__ x, const float *__restrict__ w,
                                                        const float *__restrict__ b, float *__restrict__ out,
                                                        float *__restrict__ w11, int H, int W, int tilesX, int tilesY)
{
    __shared__ float ws[64 * 9], bs[64];
    for (int i = threadIdx.x; i < 64 * 9; i += CX * CY) {
        const int m = i / 9, t = i - 9 * m;
        const float s = (w[(m * 3 + 0) * 9 + t] + w[(m * 3 + 1) * 9 + t]) + w[(m * 3 + 2) * 9 + t];
        ws[i] = s;
        if (w11 && blockIdx.x == 0) w11[i] = s;                // the summed filters, for the backward's synthesis
    }
    if (threadIdx.x < 64) bs[threadIdx.x] = b[threadIdx.x];
    __syncthreads();
    int r = blockIdx.x;
    const int tx = r % tilesX; r /= tilesX;
    const int ty = r % tilesY, p = r / tilesY;
    const int X = tx * CX + (threadIdx.x % CX), Y = ty * CY + (int)(threadIdx.x / CX);
    if (X >= W || Y >= H) return;
    const size_t plane = (size_t)H * W;
    const float *xp = x + (size_t)p * plane;
    float nb[9];
#pragma unroll
    for (int ki = 0; ki < 3; ++ki)
#pragma unroll
        for (int kj = 0; kj < 3; ++kj) {
            const int yy = Y + ki - 1, xx = X + kj - 1;
            nb[ki * 3 + kj] = (yy >= 0 && yy < H && xx >= 0 && xx < W) ? xp[(size_t)yy * W + xx] : 0.0f;
        }
    float *o = out + (size_t)p * 64 * plane + (size_t)Y * W + X;
#pragma unroll 4
    for (int m = 0; m < 64; ++m) {
        float acc = bs[m];
#pragma unroll
        for (int t = 0; t < 9; ++t) acc = fmaf(ws[m * 9 + t], nb[t], acc);
        o[(size_t)m * plane] = fmaxf(acc, 0.0f);
    }
}

__global__ __launch_bounds__(256) void k_vgg_fold(const double *__restrict__ partial, int n, double inv_count,
                                                  float *__restrict__ loss)
{
    __shared__ double red[256];
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) s += partial[i];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) loss[0] = (float)(red[0] * inv_count);
}

__global__ __launch_bounds__(256) void k_vgg_scale(float *__restrict__ dx, float *__restrict__ dy, size_t n,
                                                   const float *__restrict__ g, float c)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float s = c * g[0];
    if (dx) dx[i] *= s;
    if (dy) dy[i] *= -s;
}

// the dense layers conv1_2 .. conv3_3: (in, out, level) with level 0 = (H, W), 1 = (H2, W2), 2 = (H4, W4)
constexpr int NL = 6;
constexpr int L_IN[NL] = {64, 64, 128, 128, 256, 256}, L_OUT[NL] = {64, 128, 128, 256, 256, 256},
              L_LEV[NL] = {0, 1, 1, 2, 2, 2};

struct Dims {
    int P, H[3], W[3];
    size_t px(int lev) const { return (size_t)P * H[lev] * W[lev]; }
};

cdl_geom layer_geom(const Dims &d, int C, int M, int lev)
{
    cdl_geom g{};
    g.N = d.P; g.C = C; g.M = M; g.D = 1; g.H = d.H[lev]; g.W = d.W[lev];
    g.Pd = 1; g.Ph = 3; g.Pw = 3; g.pd = 0; g.ph = 1; g.pw = 1; g.sd = 1; g.sh = 1; g.sw = 1;
    return g;
}

struct Set {                                   // the activations one image's backward needs
    float *a1, *p1, *a3, *p2, *a5, *a6;
    unsigned char *am1, *am2;
};

// scratch layout (floats, every part a multiple of 64): fragments | conv1_1 filters | partial sums | fy | seed x |
// seed y | 1 or 2 activation sets | two backward buffers
struct Layout {
    size_t frag, part, fy, sx, sy, set, g_a, g_b, total;
    int nparts, nsets;
    bool ok;
};

size_t up64(size_t n) { return (n + 63) & ~(size_t)63; }

size_t set_floats(const Dims &d)
{
    return up64(64 * d.px(0)) + up64(64 * d.px(1)) + up64((64 * d.px(1) + 3) / 4) + up64(128 * d.px(1)) +
           up64(128 * d.px(2)) + up64((128 * d.px(2) + 3) / 4) + 2 * up64(256 * d.px(2));
}

Set set_at(float *base, const Dims &d)
{
    Set s;
    float *q = base;
    s.a1 = q; q += up64(64 * d.px(0));
    s.p1 = q; q += up64(64 * d.px(1));
    s.am1 = reinterpret_cast<unsigned char *>(q); q += up64((64 * d.px(1) + 3) / 4);
    s.a3 = q; q += up64(128 * d.px(1));
    s.p2 = q; q += up64(128 * d.px(2));
    s.am2 = reinterpret_cast<unsigned char *>(q); q += up64((128 * d.px(2) + 3) / 4);
    s.a5 = q; q += up64(256 * d.px(2));
    s.a6 = q;
    return s;
}

bool dims_of(int P, int H, int W, Dims *d)
{
    if (P < 1 || H < 4 || W < 4) return false;
    d->P = P;
    d->H[0] = H; d->W[0] = W;
    d->H[1] = H / 2; d->W[1] = W / 2;
    d->H[2] = d->H[1] / 2; d->W[2] = d->W[1] / 2;
    return true;
}

Layout layout_of(const Dims &d, int grads)
{
    Layout L{};
    size_t frag = 0;
    for (int l = 0; l < NL; ++l) {
        const cdl_geom g = layer_geom(d, L_IN[l], L_OUT[l], L_LEV[l]);
        const size_t f0 = cdl_dense_ws_floats(&g, 0), f1 = cdl_dense_ws_floats(&g, 1);
        if (!f0 || !f1) return L;                          // off the dense tier (32-bit offsets): not supported
        frag = f0 > frag ? f0 : frag;
        frag = f1 > frag ? f1 : frag;
    }
    const cdl_geom g33 = layer_geom(d, 256, 256, 2);
    const size_t np = cdl_dense_vgg_workgroups(&g33, 0);
    if (!np || np >= ((size_t)1 << 31)) return L;
    L.nparts = (int)np;
    L.nsets = (grads & CDL_VGG_DY) ? 2 : 1;
    const size_t f3 = up64(256 * d.px(2));
    L.frag = 0;
    L.part = up64(frag) + 64 * 9;                          // then the summed conv1_1 filters (576 floats)
    L.fy = L.part + up64(2 * np);
    L.sx = L.fy + f3;
    L.sy = L.sx + f3;
    L.set = L.sy + ((grads & CDL_VGG_DY) ? f3 : 0);
    L.g_a = L.set + L.nsets * set_floats(d);
    size_t ga = 256 * d.px(2), gb = 64 * d.px(0);
    if (128 * d.px(2) > ga) ga = 128 * d.px(2);
    if (64 * d.px(1) > ga) ga = 64 * d.px(1);
    L.g_b = L.g_a + up64(ga);
    L.total = L.g_b + up64(gb > 256 * d.px(2) ? gb : 256 * d.px(2));
    L.ok = true;
    return L;
}

float *w11_of(float *scratch, const Layout &L) { return scratch + L.part - 64 * 9; }

bool weights_ok(const float *const *w, const float *const *b)
{
    if (!w || !b) return false;
    for (int l = 0; l < 7; ++l)
        if (!w[l] || !b[l]) return false;
    return true;
}

// relu3_3 of one image: into f (CDL_VGG_BIAS at conv3_3), or against fy into the seeds and partial sums (CDL_VGG_DIFF)
int features(const Dims &d, const float *img, const float *const *w, const float *const *b, const Set &s,
             float *scratch, const Layout &L, float *f, const float *fy, float *sx, float *sy, void *stream)
{
    float *ws = scratch + L.frag;
    const size_t wsn = L.part - 64 * 9 - L.frag;
    const int tilesX = (d.W[0] + CX - 1) / CX, tilesY = (d.H[0] + CY - 1) / CY;
    const size_t blocks = (size_t)d.P * tilesX * tilesY;
    if (blocks >= ((size_t)1 << 31)) return CDL_EUNSUPPORTED;
    k_vgg_conv11<<<(unsigned)blocks, CX * CY, 0, S(stream)>>>(img, w[0], b[0], s.a1, w11_of(scratch, L), d.H[0],
                                                                d.W[0], tilesX, tilesY);
    CDL_LAUNCH_CHECK();
    double *part = reinterpret_cast<double *>(scratch + L.part);
    const float *in[NL] = {s.a1, s.p1, s.a3, s.p2, s.a5, s.a6};
    float *out[NL] = {s.p1, s.a3, s.p2, s.a5, s.a6, f};
    unsigned char *arg[NL] = {s.am1, nullptr, s.am2, nullptr, nullptr, nullptr};
    const int form[NL] = {CDL_VGG_POOL, CDL_VGG_BIAS, CDL_VGG_POOL, CDL_VGG_BIAS, CDL_VGG_BIAS,
                          fy ? CDL_VGG_DIFF : CDL_VGG_BIAS};
    for (int l = 0; l < NL; ++l) {
        const cdl_geom g = layer_geom(d, L_IN[l], L_OUT[l], L_LEV[l]);
        CDL_TRY(cdl_dense_vgg(&g, 0, form[l], in[l], w[l + 1], b[l + 1], nullptr, out[l], arg[l], nullptr, fy, sx, sy,
                              part, ws, wsn, stream));
    }
    return 0;
}

// the gradient with respect to one image, up to the final scale: seed (relu3_3 level) -> dimg
int backward(const Dims &d, const float *const *w, const Set &s, const float *seed, float *scratch, const Layout &L,
             float *dimg, void *stream)
{
    float *ws = scratch + L.frag;
    const size_t wsn = L.part - 64 * 9 - L.frag;
    float *ga = scratch + L.g_a, *gb = scratch + L.g_b;
    // transposed conv3_3 .. conv1_2: x -> out, gated by the forward activation that fed the layer
    const float *in[NL] = {seed, ga, gb, ga, gb, ga};
    float *out[NL] = {ga, gb, ga, gb, ga, gb};
    const float *gate[NL] = {s.a6, s.a5, s.p2, s.a3, s.p1, nullptr};         // relu1_1's gate: in cdl_synthesis
    const unsigned char *unp[NL] = {nullptr, nullptr, nullptr, s.am2, nullptr, s.am1};
    for (int k = 0; k < NL; ++k) {
        const int l = NL - 1 - k;
        const cdl_geom g = layer_geom(d, L_IN[l], L_OUT[l], L_LEV[l]);
        CDL_TRY(cdl_dense_vgg(&g, 1, unp[k] ? CDL_VGG_UNPOOL : CDL_VGG_PLAIN, in[k], w[l + 1], nullptr, gate[k], out[k],
                              nullptr, unp[k], nullptr, nullptr, nullptr, nullptr, ws, wsn, stream));
    }
    cdl_geom g1 = layer_geom(d, 1, 64, 0);
    return cdl_synthesis(&g1, gb, s.a1, w11_of(scratch, L), 1.0f, nullptr, nullptr, dimg, nullptr, 0, stream);
}

}  // namespace

extern "C" {

size_t cdl_vgg_scratch_floats(int P, int H, int W, int grads)
{
    Dims d;
    if ((grads & ~(CDL_VGG_DX | CDL_VGG_DY)) || !dims_of(P, H, W, &d)) return 0;
    const Layout L = layout_of(d, grads);
    return L.ok ? L.total : 0;
}

int cdl_vgg_forward(const float *x, const float *y, int P, int H, int W, const float *const *w, const float *const *b,
                    int grads, float *feat, float *loss, float *scratch, size_t scratch_floats, void *stream)
{
    Dims d;
    if (!y || !weights_ok(w, b) || !scratch || !dims_of(P, H, W, &d)) return CDL_EINVAL;
    if (grads & ~(CDL_VGG_DX | CDL_VGG_DY)) return CDL_EINVAL;
    if (x ? !loss : (!feat || grads)) return CDL_EINVAL;
    const Layout L = layout_of(d, grads);
    if (!L.ok) return CDL_EUNSUPPORTED;
    if (scratch_floats < L.total || (reinterpret_cast<size_t>(scratch) & 15)) return CDL_EINVAL;
    float *fy = feat ? feat : scratch + L.fy;
    const Set s0 = set_at(scratch + L.set, d), s1 = set_at(scratch + L.set + set_floats(d), d);
    CDL_TRY(features(d, y, w, b, L.nsets == 2 ? s1 : s0, scratch, L, fy, nullptr, nullptr, nullptr, stream));
    if (!x) return 0;
    CDL_TRY(features(d, x, w, b, s0, scratch, L, nullptr, fy, scratch + L.sx,
                     (grads & CDL_VGG_DY) ? scratch + L.sy : nullptr, stream));
    const double count = 256.0 * (double)d.px(2);
    k_vgg_fold<<<1, 256, 0, S(stream)>>>(reinterpret_cast<const double *>(scratch + L.part), L.nparts, 1.0 / count,
                                         loss);
    CDL_LAUNCH_CHECK();
    return 0;
}

int cdl_vgg_backward(int P, int H, int W, const float *const *w, const float *const *b, int grads,
                     const float *g_loss, float *dx, float *dy, float *scratch, size_t scratch_floats, void *stream)
{
    Dims d;
    if (!weights_ok(w, b) || !g_loss || !scratch || !dims_of(P, H, W, &d)) return CDL_EINVAL;
    if (grads & ~(CDL_VGG_DX | CDL_VGG_DY)) return CDL_EINVAL;
    if ((!dx && !dy) || (dx && !(grads & CDL_VGG_DX)) || (dy && !(grads & CDL_VGG_DY))) return CDL_EINVAL;
    const Layout L = layout_of(d, grads);
    if (!L.ok) return CDL_EUNSUPPORTED;
    if (scratch_floats < L.total || (reinterpret_cast<size_t>(scratch) & 15)) return CDL_EINVAL;
    const Set s0 = set_at(scratch + L.set, d), s1 = set_at(scratch + L.set + set_floats(d), d);
    if (dx) CDL_TRY(backward(d, w, s0, scratch + L.sx, scratch, L, dx, stream));
    if (dy) CDL_TRY(backward(d, w, s1, scratch + L.sy, scratch, L, dy, stream));
    const size_t n = d.px(0);
    const double count = 256.0 * (double)d.px(2);
    k_vgg_scale<<<(unsigned)((n + 255) / 256), 256, 0, S(stream)>>>(dx, dy, n, g_loss, (float)(2.0 / count));
    CDL_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
