// cet.hip -- the CET text adapter beside feat_map (groundingdino_dt.py with use_cet, cet_type = "Adapter"), forward and backward
// (C ABI, the defining formulas and the reasons for what is kept: include/zira_cet.h).
//
// Every product is v_mfma_f32_32x32x2_f32 in the orientation of csrc/mfma_f32_tile.h, and every kernel that multiplies is ONE
// wave per block: lane (r, hh) of a wave that owns 32 rows holds row r.
//   * the down product is taken TRANSPOSED, h^T = W_d x^T: the hidden unit is the accumulator's row, the text row its column.
//     Register t of that accumulator is then the up product's operand as it stands (the contraction runs over the rows of the
//     previous result), so the hidden activation goes from one matrix instruction to the next without LDS and without a store;
//   * out^T = W_u h^T keeps eight 32 x 32 accumulators (128 registers a lane), column = text row: the gate's scale, a per-row
//     number, is a per-lane scalar in the epilogue, and four consecutive registers are four consecutive output columns.
// S waves share a row tile (zira_cet_splits): wave (tile, s) takes the hidden panels s, s + S, ...; partial accumulators meet in
// the workspace and the wave that draws the tile's last ticket adds them in index order.  No wave ever waits for another.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "gate.h"
#include "launch.h"
#include "mfma_f32_tile.h"
#include "ticket.h"
#include "zero_loss.h"
#include "zira_cet.h"
#include "zira_msda.h"

namespace {

constexpr int kOut = ZIRA_CET_OUT, kMaxE = ZIRA_CET_MAX_E, kMaxH = ZIRA_CET_MAX_H, kMaxG = ZIRA_CET_MAX_GATES;
constexpr int kTileRows = 32, kOutTiles = kOut / 32;
constexpr int kFill = 512;                           // waves the forward and the hidden pass aim for
constexpr int kPrepWaves = 4, kPrepThreads = 64 * kPrepWaves, kPrepRows = kTileRows / kPrepWaves;
constexpr int kGateSlots = kMaxE / 64;               // columns of x a lane of the row pass holds
constexpr int kFoldThreads = 256;
using zira::align4, zira::misaligned, zira::tiles_of;

// gs[g][:] = gate[g] / |gate[g]|, ginv[g] = 1 / |gate[g]| for g < G.  Wave `wave` of `nwaves` takes rows wave, wave + nwaves, ...
__device__ __forceinline__ void normalise_gate(const float *__restrict__ gate, int G, int E, float *gs, float *ginv, int wave,
                                               int nwaves, int lane)
{
    for (int g = wave; g < G; g += nwaves) {
        float ss = 0.f;
        for (int k = lane; k < E; k += 64) {
            const float v = gate[(size_t)g * E + k];
            ss = fmaf(v, v, ss);
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) ss += __shfl_xor(ss, o, 64);
        const float n = sqrtf(ss);
        for (int k = lane; k < E; k += 64) gs[g * E + k] = gate[(size_t)g * E + k] / n;
        if (lane == 0) ginv[g] = 1.f / n;
    }
}

// the panel's h^T before bias and ReLU: a0 + a1 = W_d[panel] x^T over E, even and odd slices of 32 in chains of their own.
// xrow: row r of x, wrow: row (panel's first unit + r) of W_d
__device__ __forceinline__ void down_panel(const float *__restrict__ xrow, const float *__restrict__ wrow, int E, int hh,
                                           f32x16 &a0, f32x16 &a1)
{
    const int ns = E >> 5;
    for (int c = 0; c < ns; c += 2) {
        float wa[16], xb[16];
        load_floats(wrow + 32 * c + 16 * hh, wa);
        load_floats(xrow + 32 * c + 16 * hh, xb);
        mfma_chain<16>(wa, xb, a0);
        if (c + 1 < ns) {
            float wa2[16], xb2[16];
            load_floats(wrow + 32 * c + 32 + 16 * hh, wa2);
            load_floats(xrow + 32 * c + 32 + 16 * hh, xb2);
            mfma_chain<16>(wa2, xb2, a1);
        }
    }
}

// relu(a0 + a1 + b_d) of the panel; register 4 q + e is hidden unit hid0 + 8 q + 4 hh + e
__device__ __forceinline__ f32x16 hidden_of(const f32x16 &a0, const f32x16 &a1, const float *__restrict__ bd, int hid0, int hh)
{
    f32x16 hv;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const float4 b = *reinterpret_cast<const float4 *>(bd + hid0 + 8 * q + 4 * hh);
        const float bb[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float v = (a0[4 * q + e] + a1[4 * q + e]) + bb[e];
            hv[4 * q + e] = v < 0.f ? 0.f : v;
        }
    }
    return hv;
}

// (zero_loss.h's SmoothL1 beside L1 and L2 under one switch, |o| taken once ahead of it: calling into the header is other code)
__device__ __forceinline__ float loss_of(float o, int loss_type)
{
    const float a = fabsf(o);
    if (loss_type == ZIRA_CET_LOSS_L1) return a;
    if (loss_type == ZIRA_CET_LOSS_L2) return o * o;
    return a < 1.f ? 0.5f * o * o : a - 0.5f;
}

__device__ __forceinline__ float loss_slope(float o, int loss_type)
{
    if (loss_type == ZIRA_CET_LOSS_L1) return sign_of(o);
    if (loss_type == ZIRA_CET_LOSS_L2) return 2.f * o;
    return fabsf(o) < 1.f ? o : sign_of(o);
}

__global__ __launch_bounds__(64) void cet_fwd(const float *__restrict__ x, const float *__restrict__ feat,
                                              const float *__restrict__ Wd, const float *__restrict__ bd,
                                              const float *__restrict__ Wu, const float *__restrict__ bu,
                                              const float *__restrict__ gate, int M, int E, int H, int G, float gate_T, float base,
                                              int loss_type, int S, double inv_n, float *__restrict__ enc, float *__restrict__ loss,
                                              float *__restrict__ out, float *scale_out, int32_t *__restrict__ amax_out,
                                              float *__restrict__ cos_out, float *__restrict__ rnorm_out, float *part_out,
                                              double *part_loss, unsigned *tickets)
{
    __shared__ __align__(16) float gs[kMaxG * kMaxE];
    __shared__ float ginv[kMaxG];

    const int lane = threadIdx.x, r = lane & 31, hh = lane >> 5;
    const int tile = blockIdx.x, tiles = gridDim.x, s = blockIdx.y;
    const int row = tile * kTileRows + r, rowc = row < M ? row : M - 1;      // (rows beyond M: clamped for the loads, never stored)
    const float *xrow = x + (size_t)rowc * E;

    // ---- the gate: wave 0 of the tile, from the rows it is about to multiply ---------------------------------------------------------
    float scale = base;
    if (s == 0) {
        int amax = 0;
        float cmax = 0.f, rn = 0.f;
        if (G > 0) {
            normalise_gate(gate, G, E, gs, ginv, 0, 1, lane);
            __syncthreads();
            float ss = 0.f, dg[kMaxG];
#pragma unroll
            for (int g = 0; g < kMaxG; ++g) dg[g] = 0.f;
            for (int c = 0; c < (E >> 5); ++c) {
                const int k0 = 32 * c + 16 * hh;
                float xb[16];
                load_floats(xrow + k0, xb);
                float ss_l = 0.f;
#pragma unroll
                for (int t = 0; t < 16; ++t) ss_l = fmaf(xb[t], xb[t], ss_l);
                ss += ss_l;
#pragma unroll
                for (int g = 0; g < kMaxG; ++g)
                    if (g < G) {
                        float d = 0.f;
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            const float4 gv = *reinterpret_cast<const float4 *>(gs + g * E + k0 + 4 * i);
                            d = fmaf(xb[4 * i], gv.x, d); d = fmaf(xb[4 * i + 1], gv.y, d);
                            d = fmaf(xb[4 * i + 2], gv.z, d); d = fmaf(xb[4 * i + 3], gv.w, d);
                        }
                        dg[g] += d;
                    }
            }
            ss += xhalf(ss);
#pragma unroll
            for (int g = 0; g < kMaxG; ++g) dg[g] += xhalf(dg[g]);
            const float norm = sqrtf(ss);
            cmax = dg[0] / norm;
#pragma unroll
            for (int g = 1; g < kMaxG; ++g)
                if (g < G) {
                    const float cg = dg[g] / norm;
                    if (cg > cmax) { cmax = cg; amax = g; }      // strictly greater: the first index on a tie
                }
            scale = base * (1.f / (1.f + expf(-gate_T * cmax)));
            rn = 1.f / norm;
        }
        if (hh == 0 && row < M) {
            scale_out[row] = scale; amax_out[row] = amax; cos_out[row] = cmax; rnorm_out[row] = rn;
        }
    }

    // ---- the wave's hidden panels: down product, bias, ReLU, and straight into the up product ------------------------------------------
    f32x16 o[kOutTiles];
#pragma unroll
    for (int j = 0; j < kOutTiles; ++j) o[j] = zero16();
    const int npanels = H >> 5;
    for (int p = s; p < npanels; p += S) {
        const int hid0 = 32 * p;
        f32x16 a0 = zero16(), a1 = zero16();
        down_panel(xrow, Wd + (size_t)(hid0 + r) * E, E, hh, a0, a1);
        const f32x16 hv = hidden_of(a0, a1, bd, hid0, hh);
#pragma unroll
        for (int j = 0; j < kOutTiles; ++j) {
            float wa[16];                                        // W_u[32 j + r] at the hidden units of hv's registers
            load_tile(Wu + (size_t)(32 * j + r) * H, hid0, hh, wa);
            mfma_chain<16>(wa, hv, o[j]);
        }
    }

    // ---- S > 1: the partial accumulators meet; the wave that draws the tile's last ticket adds them in index order --------------------
    if (S > 1) {
        float *mine = part_out + ((size_t)(s * tiles + tile) * kTileRows + r) * kOut;
#pragma unroll
        for (int j = 0; j < kOutTiles; ++j) store_tile(mine, 32 * j, hh, o[j]);
        release_agent();
        if (!drew_last(tickets + 1 + tile, (unsigned)S - 1, lane)) return;
        acquire_agent();
        scale = scale_out[rowc];
        // (load_tile's map a quad at a time, one loop over the S partials per 16-byte access: a whole tile per loop is other code)
#pragma unroll
        for (int j = 0; j < kOutTiles; ++j)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
                for (int t = 0; t < S; ++t) {
                    const float4 v = *reinterpret_cast<const float4 *>(part_out + ((size_t)(t * tiles + tile) * kTileRows + r) * kOut
                                                                       + 32 * j + 8 * q + 4 * hh);
                    acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
                }
                o[j][4 * q] = acc.x; o[j][4 * q + 1] = acc.y; o[j][4 * q + 2] = acc.z; o[j][4 * q + 3] = acc.w;
            }
    }

    // ---- epilogue: bias, gate, feat; the tile's sum of L(out) ---------------------------------------------------------------------------
    double lsum = 0.0;
#pragma unroll
    for (int j = 0; j < kOutTiles; ++j)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int n = 32 * j + 8 * q + 4 * hh;
            const float4 b = *reinterpret_cast<const float4 *>(bu + n);
            const float4 v = make_float4((o[j][4 * q] + b.x) * scale, (o[j][4 * q + 1] + b.y) * scale,
                                         (o[j][4 * q + 2] + b.z) * scale, (o[j][4 * q + 3] + b.w) * scale);
            if (row < M) {
                const float4 f = *reinterpret_cast<const float4 *>(feat + (size_t)row * kOut + n);
                *reinterpret_cast<float4 *>(out + (size_t)row * kOut + n) = v;
                *reinterpret_cast<float4 *>(enc + (size_t)row * kOut + n) = make_float4(f.x + v.x, f.y + v.y, f.z + v.z, f.w + v.w);
                if (loss_type != ZIRA_CET_LOSS_NONE) {
                    lsum += (double)loss_of(v.x, loss_type); lsum += (double)loss_of(v.y, loss_type);
                    lsum += (double)loss_of(v.z, loss_type); lsum += (double)loss_of(v.w, loss_type);
                }
            }
        }
    if (loss_type == ZIRA_CET_LOSS_NONE) {
        if (tile == 0 && lane == 0) loss[0] = 0.f;
        return;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) lsum += __shfl_xor(lsum, off, 64);      // (lane_sum_xor64, inline: the call is other code)
    if (lane == 0) part_loss[tile] = lsum;
    release_agent();
    if (!drew_last(tickets, (unsigned)tiles - 1, lane)) return;
    acquire_agent();
    if (lane == 0) {
        double total = 0.0;
#pragma unroll 8
        for (int i = 0; i < tiles; ++i) total += part_loss[i];
        loss[0] = (float)(total * inv_n);
    }
}

// The backward's row pass: a block of four waves owns a row tile, a wave eight of its rows, a lane four output columns and up
// to twelve columns of x.  gu = g_out * scale; the gate's part of gx; per tile, as doubles: g_b_up [256] and g_gate [G, E].
__global__ __launch_bounds__(kPrepThreads) void cet_bwd_prep(const float *__restrict__ g_enc, const float *__restrict__ g_loss,
                                                             const float *__restrict__ x, const float *__restrict__ out,
                                                             const float *__restrict__ scale, const int32_t *__restrict__ amax,
                                                             const float *__restrict__ cosv, const float *__restrict__ rnorm,
                                                             const float *__restrict__ gate, int M, int E, int G, float gate_T,
                                                             float base, int loss_type, float inv_n, float *__restrict__ gu,
                                                             float *__restrict__ gx, double *__restrict__ part)
{
    __shared__ __align__(16) float gs[kMaxG * kMaxE];
    __shared__ float ginv[kMaxG];
    __shared__ __align__(16) float acc[kOut + kMaxG * kMaxE];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (G > 0) normalise_gate(gate, G, E, gs, ginv, wave, kPrepWaves, lane);
    __syncthreads();
    const float s = (loss_type != ZIRA_CET_LOSS_NONE && g_loss != nullptr) ? g_loss[0] * inv_n : 0.f;

    float4 gbu = make_float4(0.f, 0.f, 0.f, 0.f);
    float gg[kMaxG][kGateSlots];
#pragma unroll
    for (int g = 0; g < kMaxG; ++g)
#pragma unroll
        for (int m = 0; m < kGateSlots; ++m) gg[g][m] = 0.f;

    for (int rr = 0; rr < kPrepRows; ++rr) {
        const int row = (int)blockIdx.x * kTileRows + wave * kPrepRows + rr;
        if (row >= M) break;                                           // (the same for every lane of the wave)
        const size_t at = (size_t)row * kOut + 4 * lane;
        const float4 o = *reinterpret_cast<const float4 *>(out + at);
        float4 go = g_enc != nullptr ? *reinterpret_cast<const float4 *>(g_enc + at) : make_float4(0.f, 0.f, 0.f, 0.f);
        if (s != 0.f) {
            go.x += loss_slope(o.x, loss_type) * s; go.y += loss_slope(o.y, loss_type) * s;
            go.z += loss_slope(o.z, loss_type) * s; go.w += loss_slope(o.w, loss_type) * s;
        }
        const float sc = scale[row];
        const float4 g4 = make_float4(go.x * sc, go.y * sc, go.z * sc, go.w * sc);
        *reinterpret_cast<float4 *>(gu + at) = g4;
        gbu.x += g4.x; gbu.y += g4.y; gbu.z += g4.z; gbu.w += g4.w;
        if (G > 0) {
            float dot = fmaf(go.x, o.x, fmaf(go.y, o.y, fmaf(go.z, o.z, go.w * o.w)));
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) dot += __shfl_xor(dot, off, 64);
            int id = __builtin_amdgcn_readfirstlane(amax[row]);
            id = id < 0 ? 0 : (id >= G ? G - 1 : id);
            const float g_c = (dot / sc) * gate_T * sc * (1.f - sc / base), rn = rnorm[row], c = cosv[row], gi = ginv[id];
            const GateCoeffs co = gate_backward_coeffs(g_c, c, rn, gi);
#pragma unroll
            for (int m = 0; m < kGateSlots; ++m) {
                const int k = lane + 64 * m;
                if (k < E) {
                    const float xv = x[(size_t)row * E + k], gv = gs[id * E + k];
                    if (gx != nullptr) gx[(size_t)row * E + k] = fmaf(co.a, gv, co.b * xv);
                    const float d = fmaf(co.alpha, xv, co.beta * gv);
#pragma unroll
                    for (int g = 0; g < kMaxG; ++g)
                        if (id == g) gg[g][m] += d;
                }
            }
        } else if (gx != nullptr) {
            for (int k = lane; k < E; k += 64) gx[(size_t)row * E + k] = 0.f;
        }
    }

    // the four waves' sums, added in wave order through LDS; then the tile's doubles
    for (int w = 0; w < kPrepWaves; ++w) {
        if (wave == w) {
            float4 *dst = reinterpret_cast<float4 *>(acc + 4 * lane);
            if (w == 0) *dst = gbu;
            else { const float4 v = *dst; *dst = make_float4(v.x + gbu.x, v.y + gbu.y, v.z + gbu.z, v.w + gbu.w); }
#pragma unroll
            for (int g = 0; g < kMaxG; ++g)
#pragma unroll
                for (int m = 0; m < kGateSlots; ++m) {
                    const int k = lane + 64 * m;
                    if (g < G && k < E) {
                        float *d = acc + kOut + g * E + k;
                        *d = w == 0 ? gg[g][m] : *d + gg[g][m];
                    }
                }
        }
        __syncthreads();
    }
    const int n1 = kOut + G * E;
    for (int e = tid; e < n1; e += kPrepThreads) part[(size_t)blockIdx.x * n1 + e] = (double)acc[e];
}

// The backward's hidden pass, with the forward's split: h again (the same instructions in the same order: the same bits),
// gh = (gu W_u) o [h > 0], both stored for the weight gradients' tall products; per tile, as doubles: g_b_down [H].
__global__ __launch_bounds__(64) void cet_bwd_hidden(const float *__restrict__ x, const float *__restrict__ gu,
                                                     const float *__restrict__ Wd, const float *__restrict__ bd,
                                                     const float *__restrict__ Wu, int M, int E, int H, int S,
                                                     float *__restrict__ h_out, float *__restrict__ gh_out, double *__restrict__ part)
{
    const int lane = threadIdx.x, r = lane & 31, hh = lane >> 5;
    const int tile = blockIdx.x, s = blockIdx.y;
    const int row = tile * kTileRows + r, rowc = row < M ? row : M - 1;
    const float *xrow = x + (size_t)rowc * E, *grow = gu + (size_t)rowc * kOut;
    const int npanels = H >> 5;
    for (int p = s; p < npanels; p += S) {
        const int hid0 = 32 * p;
        f32x16 a0 = zero16(), a1 = zero16();
        down_panel(xrow, Wd + (size_t)(hid0 + r) * E, E, hh, a0, a1);
        const f32x16 hv = hidden_of(a0, a1, bd, hid0, hh);
        // (g_h^T = W_u^T g^T as in lora_bwd_gh, and store_tile's map a quad at a time: shared spellings are other machine code)
        f32x16 g0 = zero16(), g1 = zero16();
#pragma unroll
        for (int c = 0; c < kOut / 32; ++c) {
            const int k0 = 32 * c + 16 * hh;
            float wa[16], gb[16];
            load_floats(grow + k0, gb);
#pragma unroll
            for (int t = 0; t < 16; ++t) wa[t] = Wu[(size_t)(k0 + t) * H + hid0 + r];
            mfma_chain<16>(wa, gb, (c & 1) ? g1 : g0);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            float ghv[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) ghv[e] = hv[4 * q + e] > 0.f ? g0[4 * q + e] + g1[4 * q + e] : 0.f;
            const int hid = hid0 + 8 * q + 4 * hh;
            if (row < M) {
                *reinterpret_cast<float4 *>(h_out + (size_t)row * H + hid) = make_float4(hv[4 * q], hv[4 * q + 1], hv[4 * q + 2], hv[4 * q + 3]);
                *reinterpret_cast<float4 *>(gh_out + (size_t)row * H + hid) = make_float4(ghv[0], ghv[1], ghv[2], ghv[3]);
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                double v = row < M ? (double)ghv[e] : 0.0;
#pragma unroll
                for (int off = 16; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);      // (the 32 rows of one half)
                if (r == 0) part[(size_t)tile * H + hid + e] = v;
            }
        }
    }
}

// gx += gh W_d: a wave owns 32 rows and 32 columns of x; the row pass has written the gate's part (or zeros) before
__global__ __launch_bounds__(64) void cet_bwd_gx(const float *__restrict__ gh, const float *__restrict__ Wd, int M, int E, int H,
                                                 float *__restrict__ gx)
{
    const int lane = threadIdx.x, r = lane & 31, hh = lane >> 5;
    const int row0 = (int)blockIdx.x * kTileRows, e0 = 32 * (int)blockIdx.y;
    const int rowc = row0 + r < M ? row0 + r : M - 1;
    const float *grow = gh + (size_t)rowc * H;
    f32x16 a0 = zero16(), a1 = zero16();
    const int ns = H >> 5;
    for (int c = 0; c < ns; c += 2) {
        float ga[16], wb[16];
        load_floats(grow + 32 * c + 16 * hh, ga);
#pragma unroll
        for (int t = 0; t < 16; ++t) wb[t] = Wd[(size_t)(32 * c + 16 * hh + t) * E + e0 + r];
        mfma_chain<16>(ga, wb, a0);
        if (c + 1 < ns) {
            float ga2[16], wb2[16];
            load_floats(grow + 32 * c + 32 + 16 * hh, ga2);
#pragma unroll
            for (int t = 0; t < 16; ++t) wb2[t] = Wd[(size_t)(32 * c + 32 + 16 * hh + t) * E + e0 + r];
            mfma_chain<16>(ga2, wb2, a1);
        }
    }
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
        const int rw = row0 + rowmap(reg, hh);
        if (rw < M) gx[(size_t)rw * E + e0 + r] += a0[reg] + a1[reg];
    }
}

// (the structure of adapter_bwd_fold; one kernel template for both came out as other machine code)
// element e of [g_b_up 256 | g_gate G * E | g_b_down H]: the sum over the tiles' doubles in index order.  A block folds 16
// elements: 16 groups of threads each add every 16th tile's partial, LDS joins the groups in a fixed order.
__global__ __launch_bounds__(kFoldThreads) void cet_bwd_fold(const double *__restrict__ part1, const double *__restrict__ part2,
                                                             int tiles, int n1, int H, float *__restrict__ g_bu,
                                                             float *__restrict__ g_gate, float *__restrict__ g_bd)
{
    __shared__ double red[16][16];
    const int o = threadIdx.x % 16, cg = threadIdx.x / 16, e = (int)blockIdx.x * 16 + o;
    double s = 0.0;
    if (e < n1 + H) {
        const double *src = e < n1 ? part1 + e : part2 + (e - n1);
        const size_t stride = e < n1 ? (size_t)n1 : (size_t)H;
        for (int b = cg; b < tiles; b += 16) s += src[(size_t)b * stride];
    }
    red[cg][o] = s;
    __syncthreads();
    if (cg == 0 && e < n1 + H) {
        for (int g = 1; g < 16; ++g) s += red[g][o];
        if (e < kOut) g_bu[e] = (float)s;
        else if (e < n1) g_gate[e - kOut] = (float)s;
        else g_bd[e - n1] = (float)s;
    }
}

inline bool shape_ok(long long M, int E, int H, int G)
{
    return M >= 1 && M <= ZIRA_CET_MAX_ROWS && E >= 32 && E <= kMaxE && E % 32 == 0 && H >= 32 && H <= kMaxH && H % 32 == 0
           && G >= 0 && G <= kMaxG;
}

inline int splits_of(long long M, int H)
{
    int S = kFill / tiles_of(M, kTileRows);
    if (S < 1) S = 1;
    return S > H / 32 ? H / 32 : S;
}

// backward workspace (floats): [the row pass's doubles][the hidden pass's doubles][zira_xty_f32's scratch]
struct BwdLayout {
    size_t part1, part2, xty, total;
};
inline BwdLayout bwd_layout(long long M, int E, int H, int G)
{
    BwdLayout l;
    const size_t tiles = (size_t)tiles_of(M, kTileRows);
    l.part1 = 0;
    l.part2 = align4(2 * tiles * (size_t)(kOut + G * E));
    l.xty = l.part2 + align4(2 * tiles * (size_t)H);
    l.total = l.xty + align4(zira::max_xty_workspace(M, {{H, E}, {kOut, H}}));
    return l;
}

}  // namespace

extern "C" {

int zira_cet_supported(long long M, int E, int H, int G) { return shape_ok(M, E, H, G) ? 1 : 0; }

int zira_cet_splits(long long M, int H)
{
    if (!shape_ok(M, 32, H, 0)) return 0;
    return splits_of(M, H);
}

size_t zira_cet_ticket_words(long long M)
{
    if (M < 1 || M > ZIRA_CET_MAX_ROWS) return 0;
    return align4(1 + (size_t)tiles_of(M, kTileRows));
}

size_t zira_cet_fwd_workspace_floats(long long M, int H)
{
    if (!shape_ok(M, 32, H, 0)) return 0;
    const size_t tiles = (size_t)tiles_of(M, kTileRows), S = (size_t)splits_of(M, H);
    return align4(2 * tiles) + (S > 1 ? S * tiles * kTileRows * kOut : 0);
}

size_t zira_cet_bwd_workspace_floats(long long M, int E, int H, int G)
{
    if (!shape_ok(M, E, H, G)) return 0;
    return bwd_layout(M, E, H, G).total;
}

int zira_cet_fwd_f32(const float *x, const float *feat, const float *w_down, const float *b_down, const float *w_up,
                     const float *b_up, const float *gate, long long M, int E, int H, int G, float gate_T,
                     float gate_base_scale, int loss_type, float *enc, float *loss, float *out, float *scale, int32_t *amax,
                     float *cosv, float *rnorm, float *workspace, uint32_t *tickets, void *stream)
{
    if (!shape_ok(M, E, H, G) || (G > 0) != (gate != nullptr)) return -1;
    if (loss_type < ZIRA_CET_LOSS_NONE || loss_type > ZIRA_CET_LOSS_SMOOTH_L1) return -1;
    if (!x || !feat || !w_down || !b_down || !w_up || !b_up || !enc || !loss || !out || !scale || !amax || !cosv || !rnorm
        || !workspace || !tickets) return -1;
    if (misaligned(x) || misaligned(feat) || misaligned(w_down) || misaligned(b_down) || misaligned(w_up) || misaligned(b_up)
        || misaligned(gate) || misaligned(enc) || misaligned(out) || misaligned(workspace) || misaligned(tickets)) return -1;
    const int tiles = tiles_of(M, kTileRows), S = splits_of(M, H);
    double *part_loss = reinterpret_cast<double *>(workspace);
    float *part_out = workspace + align4(2 * (size_t)tiles);
    const double inv_n = 1.0 / ((double)M * (double)kOut);
    hipLaunchKernelGGL(cet_fwd, dim3((unsigned)tiles, (unsigned)S), dim3(64), 0, (hipStream_t)stream, x, feat, w_down, b_down, w_up,
                       b_up, gate, (int)M, E, H, G, gate_T, gate_base_scale, loss_type, S, inv_n, enc, loss, out, scale, amax, cosv,
                       rnorm, part_out, part_loss, tickets);
    return (int)hipGetLastError();
}

int zira_cet_bwd_f32(const float *grad_enc, const float *grad_loss, const float *x, const float *out, const float *scale,
                     const int32_t *amax, const float *cosv, const float *rnorm, const float *w_down, const float *b_down,
                     const float *w_up, const float *gate, long long M, int E, int H, int G, float gate_T,
                     float gate_base_scale, int loss_type, float *h, float *gh, float *gu, float *gx, float *g_w_down,
                     float *g_b_down, float *g_w_up, float *g_b_up, float *g_gate, float *workspace, void *stream)
{
    if (!shape_ok(M, E, H, G) || (G > 0) != (gate != nullptr) || (G > 0) != (g_gate != nullptr)) return -1;
    if (loss_type < ZIRA_CET_LOSS_NONE || loss_type > ZIRA_CET_LOSS_SMOOTH_L1) return -1;
    if (!x || !out || !scale || !amax || !cosv || !rnorm || !w_down || !b_down || !w_up || !h || !gh || !gu || !g_w_down
        || !g_b_down || !g_w_up || !g_b_up || !workspace) return -1;
    if (misaligned(grad_enc) || misaligned(x) || misaligned(out) || misaligned(w_down) || misaligned(b_down) || misaligned(w_up)
        || misaligned(gate) || misaligned(h) || misaligned(gh) || misaligned(gu) || misaligned(gx) || misaligned(g_w_down)
        || misaligned(g_w_up) || misaligned(workspace)) return -1;
    const BwdLayout l = bwd_layout(M, E, H, G);
    const int tiles = tiles_of(M, kTileRows), S = splits_of(M, H), n1 = kOut + G * E;
    double *part1 = reinterpret_cast<double *>(workspace + l.part1), *part2 = reinterpret_cast<double *>(workspace + l.part2);
    float *xws = workspace + l.xty;
    hipStream_t st = (hipStream_t)stream;
    // ATen's mean backward divides by a host scalar: on the device that is a product with the fp32 reciprocal
    const float inv_n = 1.0f / (float)(M * kOut);
    hipLaunchKernelGGL(cet_bwd_prep, dim3((unsigned)tiles), dim3(kPrepThreads), 0, st, grad_enc, grad_loss, x, out, scale, amax, cosv,
                       rnorm, gate, (int)M, E, G, gate_T, gate_base_scale, loss_type, inv_n, gu, gx, part1);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(cet_bwd_hidden, dim3((unsigned)tiles, (unsigned)S), dim3(64), 0, st, x, gu, w_down, b_down, w_up, (int)M, E, H,
                       S, h, gh, part2);
    e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(cet_bwd_fold, dim3((unsigned)((n1 + H + 15) / 16)), dim3(kFoldThreads), 0, st, part1, part2, tiles, n1, H,
                       g_b_up, g_gate, g_b_down);
    e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    int rc = zira_xty_f32(gh, x, 1, (int)M, H, E, 0, g_w_down, xws, stream);            // g_W_down [H, E] = gh^T x
    if (rc != 0) return rc;
    rc = zira_xty_f32(gu, h, 1, (int)M, kOut, H, 0, g_w_up, xws, stream);               // g_W_up [256, H] = gu^T h
    if (rc != 0) return rc;
    if (gx != nullptr) {
        hipLaunchKernelGGL(cet_bwd_gx, dim3((unsigned)tiles, (unsigned)(E / 32)), dim3(64), 0, st, gh, w_down, (int)M, E, H, gx);
        return (int)hipGetLastError();
    }
    return 0;
}

}  // extern "C"
