// lora.hip -- the low-rank language side branch beside feat_map (RepZeroLoRA of models/GroundingDINO/adapter.py:227-259 in training
// mode), forward and backward (C ABI, the defining formulas and the reasons for what is kept: include/zira_lora.h).
//
// Every product is v_mfma_f32_32x32x2_f32 in the orientation of csrc/mfma_f32_tile.h, and every kernel that multiplies is ONE
// wave per block: lane (r, hh) of a wave that owns 32 rows holds row r.
//   * h^T = W_d x^T and twin^T = W_t x^T are taken TRANSPOSED from the same registers of x: the hidden or output unit is the
//     accumulator's row, the text row its column;
//   * register t of h^T is then the operand of out^T = W_u h^T as it stands (the contraction runs over the rows of the previous
//     result), so the hidden activation goes from one matrix instruction to the next without LDS; four consecutive registers of
//     out^T and twin^T are four consecutive output columns of one text row, and the epilogue is per lane.
// S waves share a row tile (zira_lora_splits): wave (tile, s) takes a run of the in_features panels; partial h and twin meet in
// the workspace and the wave that draws the tile's last ticket adds them in index order.  No wave ever waits for another.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "lane_sum.h"
#include "launch.h"
#include "mfma_f32_tile.h"
#include "ticket.h"
#include "zero_loss.h"
#include "zira_lora.h"
#include "zira_msda.h"

namespace {

constexpr int kOut = ZIRA_LORA_OUT, kMaxE = ZIRA_LORA_MAX_E, kMaxR = ZIRA_LORA_MAX_R;
constexpr int kTileRows = 32, kOutTiles = kOut / 32;
constexpr int kFill = 256;                           // waves the forward aims for
constexpr int kFoldThreads = 256;
using zira::align4, zira::misaligned, zira::tiles_of;

// the S partial tiles at column col0 of row (tile, r), added in index order
__device__ __forceinline__ f32x16 summed_tile(const float *part, int col0, int W, int S, int tiles, int tile, int r, int hh)
{
    double acc[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.0;
    for (int t = 0; t < S; ++t) {
        f32x16 v;
        load_tile(part + ((size_t)(t * tiles + tile) * kTileRows + r) * W, col0, hh, v);
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[e] += (double)v[e];
    }
    f32x16 a;
#pragma unroll
    for (int e = 0; e < 16; ++e) a[e] = (float)acc[e];
    return a;
}

// o = the 32 x 32 tile j of (W_u h^T): HP chains of 16 over the hidden panels in index order.  The forward and the backward
// both call this on the same h: the same instructions in the same order, the same bits
template <int HP>
__device__ __forceinline__ f32x16 up_tile(const float *__restrict__ Wu, const f32x16 (&ha)[HP], int j, int r, int hh)
{
    f32x16 o = zero16();
#pragma unroll
    for (int p = 0; p < HP; ++p) {
        f32x16 wa;                                           // W_u[32 j + r] at the hidden units of h^T's registers
        load_tile(Wu + (size_t)(32 * j + r) * (32 * HP), 32 * p, hh, wa);
        mfma_chain<16>(wa, ha[p], o);
    }
    return o;
}

// HP = R / 32 hidden panels.  part: [S][tiles][32 rows][R + 256] partial h | twin; part_loss: [tiles][2] doubles
template <int HP>
__global__ __launch_bounds__(64) void lora_fwd(const float *__restrict__ x, const float *__restrict__ Wd,
                                               const float *__restrict__ Wu, const float *__restrict__ Wt,
                                               const float *__restrict__ scaling, int M, int E, int S, int per, double inv_n,
                                               float *__restrict__ out, float *__restrict__ loss, float *__restrict__ h_out,
                                               float *part, double *part_loss, unsigned *tickets)
{
    constexpr int R = 32 * HP, W = R + kOut;
    const int lane = threadIdx.x, r = lane & 31, hh = lane >> 5;
    const int tile = blockIdx.x, tiles = gridDim.x, s = blockIdx.y;
    const int row = tile * kTileRows + r, rowc = row < M ? row : M - 1;      // (rows beyond M: clamped for the loads, never stored)
    const float *xrow = x + (size_t)rowc * E;

    // ---- the wave's panels of x, each read once: into h^T and into twin^T -------------------------------------------------------------
    f32x16 ha[HP], ta[kOutTiles];
#pragma unroll
    for (int j = 0; j < HP; ++j) ha[j] = zero16();
#pragma unroll
    for (int j = 0; j < kOutTiles; ++j) ta[j] = zero16();
    const int np = E >> 5, p1 = (s + 1) * per < np ? (s + 1) * per : np;
    for (int p = s * per; p < p1; ++p) {
        const int k0 = 32 * p + 16 * hh;
        float xb[16];
        load_floats(xrow + k0, xb);
#pragma unroll
        for (int j = 0; j < HP; ++j) {
            float wa[16];
            load_floats(Wd + (size_t)(32 * j + r) * E + k0, wa);
            mfma_chain<16>(wa, xb, ha[j]);
        }
#pragma unroll
        for (int j = 0; j < kOutTiles; ++j) {
            float wa[16];
            load_floats(Wt + (size_t)(32 * j + r) * E + k0, wa);
            mfma_chain<16>(wa, xb, ta[j]);
        }
    }

    // ---- S > 1: the partial accumulators meet; the wave that draws the tile's last ticket adds them in index order --------------------
    if (S > 1) {
        float *mine = part + ((size_t)(s * tiles + tile) * kTileRows + r) * W;
#pragma unroll
        for (int j = 0; j < HP; ++j) store_tile(mine, 32 * j, hh, ha[j]);
#pragma unroll
        for (int j = 0; j < kOutTiles; ++j) store_tile(mine, R + 32 * j, hh, ta[j]);
        release_agent();
        if (!drew_last(tickets + 1 + tile, (unsigned)S - 1, lane)) return;
        acquire_agent();
        // (in double, rounded once: h and twin then carry the error of one wave's short chains, not of S additions)
#pragma unroll
        for (int j = 0; j < HP; ++j) ha[j] = summed_tile(part, 32 * j, W, S, tiles, tile, r, hh);
#pragma unroll
        for (int j = 0; j < kOutTiles; ++j) ta[j] = summed_tile(part, R + 32 * j, W, S, tiles, tile, r, hh);
    }

    // ---- h for the backward; the up product from h^T as it stands; scale, twin, the tile's two SmoothL1 sums ----------------------------
    const float sc = scaling[0];
    if (row < M) {
#pragma unroll
        for (int j = 0; j < HP; ++j) store_tile(h_out + (size_t)row * R, 32 * j, hh, ha[j]);
    }
    double sum_b = 0.0, sum_o = 0.0;
#pragma unroll
    for (int j = 0; j < kOutTiles; ++j) {
        const f32x16 o = up_tile<HP>(Wu, ha, j, r, hh);
        f32x16 v;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const float b = sc * o[e];
            v[e] = b + ta[j][e];
            if (row < M) {
                sum_b += (double)smooth_l1_zero(b);
                sum_o += (double)smooth_l1_zero(v[e]);
            }
        }
        if (row < M) store_tile(out + (size_t)row * kOut, 32 * j, hh, v);
    }
    sum_b = lane_sum_xor64(sum_b);
    sum_o = lane_sum_xor64(sum_o);
    if (lane == 0) {
        part_loss[2 * tile] = sum_b;
        part_loss[2 * tile + 1] = sum_o;
    }
    release_agent();
    if (!drew_last(tickets, (unsigned)tiles - 1, lane)) return;
    acquire_agent();
    if (lane == 0) {
        double tb = 0.0, to = 0.0;
        for (int i = 0; i < tiles; ++i) {
            tb += part_loss[2 * i];
            to += part_loss[2 * i + 1];
        }
        loss[0] = (float)((tb + to) * inv_n);
    }
}

// The backward's element pass: wave (tile, j) owns 32 rows and the output columns 32 j ... 32 j + 31.  branch again from h
// (up_tile, the forward's bits), gt and gb stored, the wave's part of g_scaling as one double
template <int HP>
__global__ __launch_bounds__(64) void lora_bwd_rows(const float *__restrict__ g_out, const float *__restrict__ g_loss,
                                                    const float *__restrict__ out, const float *__restrict__ h,
                                                    const float *__restrict__ Wu, const float *__restrict__ scaling, int M,
                                                    float inv_n, float *__restrict__ gb, float *__restrict__ gt,
                                                    double *__restrict__ part)
{
    constexpr int R = 32 * HP;
    const int lane = threadIdx.x, r = lane & 31, hh = lane >> 5;
    const int tile = blockIdx.x, j = blockIdx.y;
    const int row = tile * kTileRows + r, rowc = row < M ? row : M - 1;
    f32x16 ha[HP];
#pragma unroll
    for (int p = 0; p < HP; ++p) load_tile(h + (size_t)rowc * R, 32 * p, hh, ha[p]);
    const f32x16 o = up_tile<HP>(Wu, ha, j, r, hh);
    const float sc = scaling[0], s = g_loss != nullptr ? g_loss[0] * inv_n : 0.f;
    f32x16 ov, go;
    load_tile(out + (size_t)rowc * kOut, 32 * j, hh, ov);
    if (g_out != nullptr) load_tile(g_out + (size_t)rowc * kOut, 32 * j, hh, go);
    else go = zero16();
    // g_scaling is ONE number out of M * 256 products that cancel: its terms are taken in double -- h W_u^T again with plain
    // double FMAs (u[e] of the lane's row and the register's column) and the element's gradient unrounded
    double u[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) u[e] = 0.0;
    for (int k = 0; k < R; k += 4) {
        const float4 hv = *reinterpret_cast<const float4 *>(h + (size_t)rowc * R + k);
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const float4 w = *reinterpret_cast<const float4 *>(Wu + (size_t)(32 * j + 8 * (e >> 2) + 4 * hh + (e & 3)) * R + k);
            u[e] = fma((double)hv.x, (double)w.x, u[e]);
            u[e] = fma((double)hv.y, (double)w.y, u[e]);
            u[e] = fma((double)hv.z, (double)w.z, u[e]);
            u[e] = fma((double)hv.w, (double)w.w, u[e]);
        }
    }
    f32x16 vt, vb;
    double gs = 0.0;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const float so = smooth_l1_zero_slope(ov[e]), sb = smooth_l1_zero_slope(sc * o[e]);
        const float t = go[e] + s * so;
        const float p = t + s * sb;
        vt[e] = t;
        vb[e] = sc * p;
        if (row < M) gs += ((double)go[e] + (double)s * ((double)so + (double)sb)) * u[e];
    }
    if (row < M) {
        store_tile(gt + (size_t)row * kOut, 32 * j, hh, vt);
        store_tile(gb + (size_t)row * kOut, 32 * j, hh, vb);
    }
    gs = lane_sum_xor64(gs);
    if (lane == 0) part[(size_t)tile * kOutTiles + j] = gs;
}

// g_h = gb W_u: wave (tile, p) owns 32 rows and the hidden units 32 p ... 32 p + 31; g_h^T = W_u^T gb^T over the 256 columns
__global__ __launch_bounds__(64) void lora_bwd_gh(const float *__restrict__ gb, const float *__restrict__ Wu, int M, int R,
                                                  float *__restrict__ gh)
{
    const int lane = threadIdx.x, r = lane & 31, hh = lane >> 5;
    const int tile = blockIdx.x, hid0 = 32 * (int)blockIdx.y;
    const int row = tile * kTileRows + r, rowc = row < M ? row : M - 1;
    const float *grow = gb + (size_t)rowc * kOut;
    // (the same body as the middle of cet_bwd_hidden; as one function the compiler commutes its address multiplies)
    f32x16 g0 = zero16(), g1 = zero16();
#pragma unroll
    for (int c = 0; c < kOut / 32; ++c) {
        const int k0 = 32 * c + 16 * hh;
        float wa[16], gv[16];
        load_floats(grow + k0, gv);
#pragma unroll
        for (int t = 0; t < 16; ++t) wa[t] = Wu[(size_t)(k0 + t) * R + hid0 + r];
        mfma_chain<16>(wa, gv, (c & 1) ? g1 : g0);
    }
    if (row < M) store_tile(gh + (size_t)row * R, hid0, hh, g0 + g1);
}

// gx = gh W_d + gt W_t: a wave owns 32 rows and 32 columns of x
__global__ __launch_bounds__(64) void lora_bwd_gx(const float *__restrict__ gh, const float *__restrict__ gt,
                                                  const float *__restrict__ Wd, const float *__restrict__ Wt, int M, int E, int R,
                                                  float *__restrict__ gx)
{
    const int lane = threadIdx.x, r = lane & 31, hh = lane >> 5;
    const int row0 = (int)blockIdx.x * kTileRows, e0 = 32 * (int)blockIdx.y;
    const int rowc = row0 + r < M ? row0 + r : M - 1;
    const float *hrow = gh + (size_t)rowc * R, *trow = gt + (size_t)rowc * kOut;
    f32x16 a0 = zero16(), a1 = zero16();
    for (int c = 0; c < (R >> 5); ++c) {
        const int k0 = 32 * c + 16 * hh;
        float ga[16], wb[16];
        load_floats(hrow + k0, ga);
#pragma unroll
        for (int t = 0; t < 16; ++t) wb[t] = Wd[(size_t)(k0 + t) * E + e0 + r];
        mfma_chain<16>(ga, wb, a0);
    }
#pragma unroll
    for (int c = 0; c < kOut / 32; ++c) {
        const int k0 = 32 * c + 16 * hh;
        float ga[16], wb[16];
        load_floats(trow + k0, ga);
#pragma unroll
        for (int t = 0; t < 16; ++t) wb[t] = Wt[(size_t)(k0 + t) * E + e0 + r];
        mfma_chain<16>(ga, wb, a1);
    }
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
        const int rw = row0 + rowmap(reg, hh);
        if (rw < M) gx[(size_t)rw * E + e0 + r] = a0[reg] + a1[reg];
    }
}

// g_scaling = the sum of the element pass's n doubles: thread i adds every 256th from i on, thread 0 adds the 256 in index order
__global__ __launch_bounds__(kFoldThreads) void lora_bwd_fold(const double *__restrict__ part, int n, float *__restrict__ g_scaling)
{
    __shared__ double red[kFoldThreads];
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += kFoldThreads) s += part[i];
    red[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int i = 1; i < kFoldThreads; ++i) s += red[i];
        g_scaling[0] = (float)s;
    }
}

inline bool shape_ok(long long M, int E, int R)
{
    return M >= 1 && M <= ZIRA_LORA_MAX_ROWS && E >= 32 && E <= kMaxE && E % 32 == 0 && R >= 32 && R <= kMaxR && R % 32 == 0;
}

// panels of 32 features a wave takes, and the waves a row tile then needs
inline int panels_per_wave(long long M, int E)
{
    const int np = E / 32;
    int smax = kFill / tiles_of(M, kTileRows);
    smax = smax < 1 ? 1 : (smax > np ? np : smax);
    return (np + smax - 1) / smax;
}
inline int splits_of(long long M, int E)
{
    const int per = panels_per_wave(M, E);
    return (E / 32 + per - 1) / per;
}

// backward workspace (floats): [the element pass's doubles][zira_xty_f32's scratch]
struct BwdLayout {
    size_t xty, total;
};
inline BwdLayout bwd_layout(long long M, int E, int R)
{
    BwdLayout l;
    l.xty = align4(2 * (size_t)tiles_of(M, kTileRows) * kOutTiles);
    l.total = l.xty + align4(zira::max_xty_workspace(M, {{kOut, E}, {R, E}, {kOut, R}}));
    return l;
}

template <int HP>
int launch_fwd(const float *x, const float *wd, const float *wu, const float *wt, const float *scaling, int M, int E, float *out,
               float *loss, float *h, float *workspace, uint32_t *tickets, hipStream_t st)
{
    const int tiles = tiles_of(M, kTileRows), S = splits_of(M, E), per = panels_per_wave(M, E);
    double *part_loss = reinterpret_cast<double *>(workspace);
    float *part = workspace + align4(4 * (size_t)tiles);
    hipLaunchKernelGGL(lora_fwd<HP>, dim3((unsigned)tiles, (unsigned)S), dim3(64), 0, st, x, wd, wu, wt, scaling, M, E, S, per,
                       1.0 / ((double)M * (double)kOut), out, loss, h, part, part_loss, tickets);
    return (int)hipGetLastError();
}

template <int HP>
int launch_bwd_rows(const float *g_out, const float *g_loss, const float *out, const float *h, const float *wu,
                    const float *scaling, int M, float *gb, float *gt, double *part, hipStream_t st)
{
    // ATen's mean backward divides by a host scalar: on the device that is a product with the fp32 reciprocal
    const float inv_n = 1.0f / (float)((long long)M * kOut);
    hipLaunchKernelGGL(lora_bwd_rows<HP>, dim3((unsigned)tiles_of(M, kTileRows), (unsigned)kOutTiles), dim3(64), 0, st, g_out,
                       g_loss, out, h, wu, scaling, M, inv_n, gb, gt, part);
    return (int)hipGetLastError();
}

// F<HP>(args...) for HP = R / 32 in 1 ... 8
#define LORA_BY_PANELS(R, F, ...)                \
    switch ((R) / 32) {                          \
    case 1: return F<1>(__VA_ARGS__);            \
    case 2: return F<2>(__VA_ARGS__);            \
    case 3: return F<3>(__VA_ARGS__);            \
    case 4: return F<4>(__VA_ARGS__);            \
    case 5: return F<5>(__VA_ARGS__);            \
    case 6: return F<6>(__VA_ARGS__);            \
    case 7: return F<7>(__VA_ARGS__);            \
    case 8: return F<8>(__VA_ARGS__);            \
    default: return -1;                          \
    }

int fwd_by_panels(int R, const float *x, const float *wd, const float *wu, const float *wt, const float *scaling, int M, int E,
                  float *out, float *loss, float *h, float *workspace, uint32_t *tickets, hipStream_t st)
{
    LORA_BY_PANELS(R, launch_fwd, x, wd, wu, wt, scaling, M, E, out, loss, h, workspace, tickets, st)
}

int bwd_rows_by_panels(int R, const float *g_out, const float *g_loss, const float *out, const float *h, const float *wu,
                       const float *scaling, int M, float *gb, float *gt, double *part, hipStream_t st)
{
    LORA_BY_PANELS(R, launch_bwd_rows, g_out, g_loss, out, h, wu, scaling, M, gb, gt, part, st)
}

}  // namespace

extern "C" {

int zira_lora_supported(long long M, int E, int R) { return shape_ok(M, E, R) ? 1 : 0; }

int zira_lora_splits(long long M, int E)
{
    if (!shape_ok(M, E, 32)) return 0;
    return splits_of(M, E);
}

size_t zira_lora_ticket_words(long long M)
{
    if (M < 1 || M > ZIRA_LORA_MAX_ROWS) return 0;
    return align4(1 + (size_t)tiles_of(M, kTileRows));
}

size_t zira_lora_fwd_workspace_floats(long long M, int E, int R)
{
    if (!shape_ok(M, E, R)) return 0;
    const size_t tiles = (size_t)tiles_of(M, kTileRows), S = (size_t)splits_of(M, E);
    return align4(4 * tiles) + (S > 1 ? S * tiles * kTileRows * (size_t)(R + kOut) : 0);
}

size_t zira_lora_bwd_workspace_floats(long long M, int E, int R)
{
    if (!shape_ok(M, E, R)) return 0;
    return bwd_layout(M, E, R).total;
}

int zira_lora_fwd_f32(const float *x, const float *w_down, const float *w_up, const float *w_twin, const float *scaling,
                      long long M, int E, int R, float *out, float *loss, float *h, float *workspace, uint32_t *tickets,
                      void *stream)
{
    if (!shape_ok(M, E, R)) return -1;
    if (!x || !w_down || !w_up || !w_twin || !scaling || !out || !loss || !h || !workspace || !tickets) return -1;
    if (misaligned(x) || misaligned(w_down) || misaligned(w_up) || misaligned(w_twin) || misaligned(out) || misaligned(h)
        || misaligned(workspace) || misaligned(tickets)) return -1;
    return fwd_by_panels(R, x, w_down, w_up, w_twin, scaling, (int)M, E, out, loss, h, workspace, tickets, (hipStream_t)stream);
}

int zira_lora_bwd_f32(const float *grad_out, const float *grad_loss, const float *x, const float *out, const float *h,
                      const float *w_down, const float *w_up, const float *w_twin, const float *scaling, long long M, int E,
                      int R, float *gb, float *gt, float *gh, float *gx, float *g_w_down, float *g_w_up, float *g_w_twin,
                      float *g_scaling, float *workspace, void *stream)
{
    if (!shape_ok(M, E, R)) return -1;
    if (!x || !out || !h || !w_down || !w_up || !w_twin || !scaling || !gb || !gt || !gh || !g_w_down || !g_w_up || !g_w_twin
        || !g_scaling || !workspace) return -1;
    if (misaligned(grad_out) || misaligned(x) || misaligned(out) || misaligned(h) || misaligned(w_down) || misaligned(w_up)
        || misaligned(w_twin) || misaligned(gb) || misaligned(gt) || misaligned(gh) || misaligned(gx) || misaligned(g_w_down)
        || misaligned(g_w_up) || misaligned(g_w_twin) || misaligned(workspace)) return -1;
    const BwdLayout l = bwd_layout(M, E, R);
    const int tiles = tiles_of(M, kTileRows);
    double *part = reinterpret_cast<double *>(workspace);
    float *xws = workspace + l.xty;
    hipStream_t st = (hipStream_t)stream;
    int rc = bwd_rows_by_panels(R, grad_out, grad_loss, out, h, w_up, scaling, (int)M, gb, gt, part, st);
    if (rc != 0) return rc;
    hipLaunchKernelGGL(lora_bwd_gh, dim3((unsigned)tiles, (unsigned)(R / 32)), dim3(64), 0, st, gb, w_up, (int)M, R, gh);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(lora_bwd_fold, dim3(1), dim3(kFoldThreads), 0, st, part, tiles * kOutTiles, g_scaling);
    e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    rc = zira_xty_f32(gb, h, 1, (int)M, kOut, R, 0, g_w_up, xws, stream);               // g_W_up [256, R] = gb^T h
    if (rc != 0) return rc;
    rc = zira_xty_f32(gh, x, 1, (int)M, R, E, 0, g_w_down, xws, stream);                // g_W_down [R, E] = gh^T x
    if (rc != 0) return rc;
    rc = zira_xty_f32(gt, x, 1, (int)M, kOut, E, 0, g_w_twin, xws, stream);             // g_W_twin [256, E] = gt^T x
    if (rc != 0) return rc;
    if (gx != nullptr) {
        hipLaunchKernelGGL(lora_bwd_gx, dim3((unsigned)tiles, (unsigned)(E / 32)), dim3(64), 0, st, gh, gt, w_down, w_twin, (int)M, E,
                           R, gx);
        return (int)hipGetLastError();
    }
    return 0;
}

}  // extern "C"
