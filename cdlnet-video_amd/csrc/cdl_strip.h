// Internal interface of the fused generic tier: the three kernels behind the cdl_fusedg_* entry points of
// include/cdlnet_hip.h and the ONE plan they share.
//   tile    k_stage_g (cdl_fusedg.hip): any C, 2-D / 3-D, unit stride, P in {3,5,7}, G = C * Pd in {1,3,5,7}, M <= 64;
//           64 x 16 pixel tiles of one (n, depth) plane, a workgroup per tile
//   strip   k_strip (cdl_strip.hip): one image channel, stride 1 or 2, up to 192 subbands -- the shipped 2-D checkpoints
//           (CDLNet-s2030: K=30 M=169 P=7 s=2, /root/reference/trained_nets/CDLNet-s2030/args.json:2-9); a wave per
//           SEG-row segment of a 32-column strip
//   stripg  k_stripg (cdl_stripg.hip): the tile kernel's shapes in the strip decomposition, reading the tile kernel's
//           prepared fragments; opt-in with CDL_FUSEDG_STRIP=1
// cdl_fusedg.hip's route_for() takes the first plan that accepts a geometry: tile (stripg in its place when switched on
// and accepting), else strip.  Whatever the entry points and size queries need is a field of the plan.
#pragma once
#include "cdl_common.h"

enum { CDL_PLAN_TILE = 0, CDL_PLAN_STRIP = 1, CDL_PLAN_STRIPG = 2 };

struct cdl_fusedg_plan {
    int kind;                        // CDL_PLAN_*
    int P, G, MT, KS, KQ;            // filter side, groups C * Pd, 32-channel tiles, 16-tap / 16-channel k-steps
    int tilesX, tilesY;              // tile: 64 x 16 tiles per plane
    int S, RT, Hz, Wz;               // strip: stride, 32-slot tap tiles, code plane
    int nsx, nsy, SEG;               // strip, stripg: 32-column strips, SEG-row segments
    int prows, pxw;                  // patch rows / columns (tile: the tile's patch; strip: per parity plane)
    int per_img;                     // work items of one sample = its rows of threshold-gradient partials
    size_t items;                    // work items = N * per_img: tiles (a workgroup each) or strip segments (a wave each)
    size_t frag_uint4;               // prepared weights of one (analysis-like, synthesis-like) pair
    size_t patch_floats, map_words;
    size_t rsc_floats;               // one code tensor in the row-strip channel-major layout CDL_LAY_RSC (tile: 0, none)
};

// What the tile and the stripg plan share: the admission rules of the grouped shapes, and P, G, MT, KS, KQ, frag_uint4
// (one fragment list serves both kernels) and map_words.
inline bool cdl_grouped_plan_base(const cdl_geom *g, cdl_fusedg_plan *pl)
{
    if (!cdl_geom_ok(g)) return false;
    if (g->sd != 1 || g->sh != 1 || g->sw != 1) return false;
    if (g->Ph != g->Pw || (g->Ph != 3 && g->Ph != 5 && g->Ph != 7)) return false;
    if ((g->Pd & 1) == 0 || g->pd != g->Pd / 2 || g->ph != g->Ph / 2 || g->pw != g->Pw / 2) return false;
    if (g->M > 64 || g->M < 8 || (g->M & 7)) return false;  // whole register quads of channels (see k_stage_g, k_stripg)
    *pl = cdl_fusedg_plan{};
    pl->P = g->Ph;
    pl->G = g->C * g->Pd;
    if (pl->G != 1 && pl->G != 3 && pl->G != 5 && pl->G != 7) return false;
    if (g->Ph == 7 && pl->G == 7) return false;             // 49 ring registers on top of the tiles: spills to scratch
    pl->S = 1;
    pl->RT = g->Ph == 7 ? 2 : 1;
    pl->MT = (g->M + 31) / 32;
    pl->KS = (pl->G * g->Ph * g->Pw + 15) / 16;
    pl->KQ = (g->M + 15) / 16;
    pl->frag_uint4 = (size_t)2 * (pl->MT * pl->KS + pl->G * pl->RT * pl->KQ) * 64;
    pl->map_words = (size_t)g->N * 4 * g->D * g->H * g->W;
    if ((size_t)g->M * g->D * g->H * g->W * 4 >= ((size_t)1 << 31)) return false;      // per-sample buffer descriptor range
    if (g->H > 65535 || (size_t)g->N * g->C * g->D > 65535) return false;               // assemble grids
    return true;
}

// ---- cdl_strip.hip
bool cdl_strip_plan_for(const cdl_geom *g, cdl_fusedg_plan *pl);
// fragments of K pairs, pair k at frags + k * frag bytes; shift2: cdl_pair_batch (cdl_common.h)
int cdl_strip_prep_pairs(const cdl_geom *g, const cdl_fusedg_plan &pl, const float *const *w1, const float *const *w2,
                         int K, int shift2, void *frags, hipStream_t st);
// mode 0: z' = ST(zin + sgn * A r, tau), 1: the same without zin, 2: reverse stage (du = [map](zin + acc), dtau);
// lay_in / lay_out: 1 = CDL_LAY_RSC
int cdl_strip_stage(const cdl_geom *g, const cdl_fusedg_plan &pl, int mode, const float *r, const float *zin,
                    const float *tau, const void *frags, float sgn, float *zout, float *patches, unsigned *map,
                    float *dtau_partial, int do_synth, int rev, int lay_in, int lay_out, hipStream_t st);
int cdl_strip_assemble(const cdl_geom *g, const cdl_fusedg_plan &pl, const float *patches, const float *mask,
                       const float *sub, float alpha, float *out, float *acc, int acc_add, hipStream_t st);

// ---- cdl_stripg.hip (fragments: the tile kernel's prep_pairs in cdl_fusedg.hip)
bool cdl_stripg_plan_for(const cdl_geom *g, cdl_fusedg_plan *pl);
// tau_planes (CDL_TAU_PER_PLANE of the entry points): tau is (N*D, M), an item reads row n * D + zd
int cdl_stripg_stage(const cdl_geom *g, const cdl_fusedg_plan &pl, int mode, const float *r, const float *zin,
                     const float *tau, const void *frags, float sgn, float *zout, float *patches, unsigned *map,
                     float *dtau_partial, int do_synth, int rev, int lay_in, int lay_out, int tau_planes, hipStream_t st);
int cdl_stripg_assemble(const cdl_geom *g, const cdl_fusedg_plan &pl, const float *patches, const float *mask,
                        const float *sub, float alpha, float *out, float *acc, int acc_add, hipStream_t st);
