// adapter.hip -- the gated bottleneck adapter beside the FFN of the deformable encoder / decoder layers, forward and backward
// (C ABI and the defining formulas: include/zira_adapter.h; reference models/GroundingDINO/adapter.py:124-179).
//
// One wave owns 32 rows, a block of four waves a panel of 128.  Every product is v_mfma_f32_32x32x2_f32 with fp32 accumulation,
// in the orientation of csrc/mfma_f32_tile.h.
// The instruction's reduction index is free as long as both operands agree on it, so lane (r, hh) holds the CONTIGUOUS 32 floats
// [64 c + 32 hh, +32) of row r of a 64-wide slice c of the left operand -- eight 16-byte loads straight from global memory, each
// row read once -- and the weight operand is read with the same index map (L2-resident: 64 KB per matrix).
//
// forward   x -> (row norm, <= 8 cosines, first arg-max, sigmoid, scale) on the vector ALU from the very registers that feed the
//           down product;  h = relu(W_d x + b_d) goes through the wave's LDS tile (accumulator layout -> operand layout) and to
//           global memory for the backward;  y = (W_u h + b_u) * scale.  sum|x| leaves each block as one double; the last block
//           to arrive (integer ticket) adds them in index order.
// backward  t = grad_y W_u (MFMA);  gh = scale * t o [h > 0];  the row's g_scale = t . h + grad_y . b_u;  gx = gh W_d (MFMA) plus
//           the gate's and the L1 term's paths in the epilogue;  a second pass over the wave's rows in row-major lanes carries
//           g_b_up and g_gate;  block sums leave as doubles and a fold kernel adds them in index order.  g_W_down = gh^T x and
//           g_W_up = grad_y^T (scale * h) are zira_xty_f32's.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "gate.h"
#include "launch.h"
#include "mfma_f32_tile.h"
#include "zira_adapter.h"
#include "zira_msda.h"

namespace {

constexpr int kD = 256, kH = 64, kMaxG = 8;
constexpr int kWaveRows = 32, kWaves = 4, kPanel = kWaveRows * kWaves, kThreads = 64 * kWaves;
constexpr int kHS = kH + 1;                          // LDS stride of a wave's [32][64] tile: operand reads and row reads conflict-free
constexpr int kPS = kWaveRows + 1;                   // LDS stride of the row-dot scratch
constexpr int kWavePart = kD + kMaxG * kD;           // g_b_up, g_gate: floats a wave carries out of the row-major pass
constexpr int kBwdPart = kH + kWavePart;             // doubles a block leaves: g_b_down, g_b_up, g_gate
constexpr long long kMaxM = 1ll << 22;
using zira::align4, zira::misaligned;

// gs[g][:] = gate[g] / |gate[g]| for g < G, zeros above; ginv[g] = 1 / |gate[g]|.  Wave w takes rows w and w + 4.
__device__ __forceinline__ void normalise_gate(const float *__restrict__ gate, int G, float *gs, float *ginv, int wave, int lane)
{
    for (int g = wave; g < kMaxG; g += kWaves) {
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (g < G) v = *reinterpret_cast<const float4 *>(gate + g * kD + 4 * lane);
        float ss = (v.x * v.x + v.y * v.y) + (v.z * v.z + v.w * v.w);
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) ss += __shfl_xor(ss, o, 64);
        const float n = sqrtf(ss);
        if (g < G) v = make_float4(v.x / n, v.y / n, v.z / n, v.w / n);
        *reinterpret_cast<float4 *>(gs + g * kD + 4 * lane) = v;
        if (lane == 0) ginv[g] = g < G ? 1.f / n : 0.f;
    }
}

__global__ __launch_bounds__(kThreads) void adapter_fwd(const float *__restrict__ x, const float *__restrict__ Wd,
                                                        const float *__restrict__ bd, const float *__restrict__ Wu,
                                                        const float *__restrict__ bu, const float *__restrict__ gate, int M, int G,
                                                        float gate_T, float base, int self_kd, float *__restrict__ y,
                                                        float *__restrict__ loss, float *__restrict__ h_out,
                                                        float *__restrict__ scale_out, int32_t *__restrict__ amax_out,
                                                        float *__restrict__ cos_out, float *__restrict__ rnorm_out, double *part,
                                                        unsigned *counter)
{
    __shared__ __align__(16) float gs[kMaxG * kD];
    __shared__ float ginv[kMaxG];
    __shared__ float hs[kWaves][kWaveRows * kHS];
    __shared__ float srow[kWaves][kWaveRows];
    __shared__ double wsum[kWaves];
    __shared__ double red[kThreads];
    __shared__ int is_last;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, hh = lane >> 5;
    const int row0 = (int)blockIdx.x * kPanel + wave * kWaveRows;
    const int row = row0 + r, rowc = row < M ? row : M - 1;        // (rows beyond M: clamped for the loads, never stored)

    normalise_gate(gate, G, gs, ginv, wave, lane);
    __syncthreads();

    // ---- down product, row statistics -------------------------------------------------------------------------------------------
    f32x16 acc[2][2];      // [column tile][chain]: even and odd slices in chains of their own, joined at the end
#pragma unroll
    for (int j = 0; j < 2; ++j) { acc[j][0] = zero16(); acc[j][1] = zero16(); }
    float ss = 0.f, ab = 0.f, dg[kMaxG];
#pragma unroll
    for (int g = 0; g < kMaxG; ++g) dg[g] = 0.f;

#pragma unroll
    for (int c = 0; c < kD / 64; ++c) {
        const int k0 = 64 * c + 32 * hh;
        float xa[32];
        load_floats(x + (size_t)rowc * kD + k0, xa);
        // the slice's sums on their own, then into the totals: no chain of additions is longer than 32 + 4
        float ss_l = 0.f, ab_l = 0.f;
#pragma unroll
        for (int t = 0; t < 32; ++t) { ss_l = fmaf(xa[t], xa[t], ss_l); ab_l += fabsf(xa[t]); }
        ss += ss_l; ab += ab_l;
#pragma unroll
        for (int g = 0; g < kMaxG; ++g)
            if (g < G) {
                float d = 0.f;
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const float4 gv = *reinterpret_cast<const float4 *>(gs + g * kD + k0 + 4 * i);     // (one address per half wave)
                    d = fmaf(xa[4 * i], gv.x, d); d = fmaf(xa[4 * i + 1], gv.y, d);
                    d = fmaf(xa[4 * i + 2], gv.z, d); d = fmaf(xa[4 * i + 3], gv.w, d);
                }
                dg[g] += d;
            }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            float wb[32];
            load_floats(Wd + (size_t)(32 * j + r) * kD + k0, wb);
            mfma_chain<32>(xa, wb, acc[j][c & 1]);
        }
    }
    // the two halves of a row meet: both lanes of the row hold the same totals afterwards
    const float ab_half = ab;
    ss += xhalf(ss);
#pragma unroll
    for (int g = 0; g < kMaxG; ++g) dg[g] += xhalf(dg[g]);
    const float norm = sqrtf(ss);
    float cmax = 0.f, scale = base;
    int amax = 0;
    if (G > 0) {
        cmax = dg[0] / norm;
#pragma unroll
        for (int g = 1; g < kMaxG; ++g)
            if (g < G) {
                const float cg = dg[g] / norm;
                if (cg > cmax) { cmax = cg; amax = g; }      // strictly greater: the first index on a tie
            }
        scale = base * (1.f / (1.f + expf(-gate_T * cmax)));
    }
    if (hh == 0) {
        srow[wave][r] = scale;
        if (row < M) {
            scale_out[row] = scale; amax_out[row] = amax; cos_out[row] = cmax; rnorm_out[row] = 1.f / norm;
        }
    }
    if (self_kd) {
        double s = row < M ? (double)ab_half : 0.0;
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o, 64);      // (lane_sum.h's lane_sum_xor64, inline: the call is other code)
        if (lane == 0) wsum[wave] = s;
    }

    // ---- h: bias, ReLU, accumulator layout -> LDS tile -> global rows and the up product's operand ----------------------------------
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const float b = bd[32 * j + r];
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const float v = (acc[j][0][reg] + acc[j][1][reg]) + b;
            hs[wave][rowmap(reg, hh) * kHS + 32 * j + r] = v < 0.f ? 0.f : v;
        }
    }
    __syncthreads();
    for (int rr = 0; rr < kWaveRows && row0 + rr < M; ++rr) h_out[(size_t)(row0 + rr) * kH + lane] = hs[wave][rr * kHS + lane];
    float ha[32];
#pragma unroll
    for (int t = 0; t < 32; ++t) ha[t] = hs[wave][r * kHS + 32 * hh + t];

    // ---- up product, two column tiles at a time ------------------------------------------------------------------------------------
#pragma unroll 1
    for (int jp = 0; jp < kD / 64; ++jp) {
        f32x16 o[2];
#pragma unroll
        for (int jj = 0; jj < 2; ++jj) {
            o[jj] = zero16();
            float wb[32];
            load_floats(Wu + (size_t)(64 * jp + 32 * jj + r) * kH + 32 * hh, wb);
            mfma_chain<32>(ha, wb, o[jj]);
        }
#pragma unroll
        for (int jj = 0; jj < 2; ++jj) {
            const int n = 64 * jp + 32 * jj + r;
            const float b = bu[n];
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const int rl = rowmap(reg, hh);
                if (row0 + rl < M) y[(size_t)(row0 + rl) * kD + n] = (o[jj][reg] + b) * srow[wave][rl];
            }
        }
    }

    // ---- loss: one double per block; the last block to arrive adds them in index order -----------------------------------------------
    if (!self_kd) {
        if (blockIdx.x == 0 && tid == 0) loss[0] = 0.f;
        return;
    }
    if (tid == 0) {      // (ticket.h's protocol in its older spelling: __threadfence() and atomic loads are other machine code)
        part[blockIdx.x] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
        __threadfence();
        const unsigned ticket = atomicInc(counter, gridDim.x - 1);       // wraps to 0 behind the last block: ready for the next call
        is_last = ticket == gridDim.x - 1;
    }
    __syncthreads();
    if (!is_last) return;
    __threadfence();
    double s = 0.0;
    for (unsigned i = tid; i < gridDim.x; i += kThreads) {
        const unsigned long long bits = __hip_atomic_load(reinterpret_cast<unsigned long long *>(part) + i, __ATOMIC_RELAXED,
                                                          __HIP_MEMORY_SCOPE_AGENT);
        s += __longlong_as_double((long long)bits);
    }
    red[tid] = s;
    __syncthreads();
    for (int o = kThreads / 2; o >= 1; o >>= 1) {
        if (tid < o) red[tid] += red[tid + o];
        __syncthreads();
    }
    if (tid == 0) loss[0] = (float)(red[0] / ((double)M * kD));
}

// LDS of the backward's row kernel, carved from one array (floats): the wave tiles of gh and the row-dot scratch are dead by the
// time the waves' sums move through the same words.
constexpr int kOffTile = 0;                                        // [kWaves][32 * kHS]
constexpr int kOffDots = kOffTile + kWaves * kWaveRows * kHS;      // [kWaves][32 * kPS]
constexpr int kScratch = kOffDots + kWaves * kWaveRows * kPS;
static_assert(kScratch >= kWaves * kWavePart, "the waves' sums reuse the tiles and the row-dot scratch");

__global__ __launch_bounds__(kThreads) void adapter_bwd_rows(const float *__restrict__ gy, const float *__restrict__ grad_loss,
                                                             const float *__restrict__ x, const float *__restrict__ h,
                                                             const float *__restrict__ scale, const int32_t *__restrict__ amax,
                                                             const float *__restrict__ cosv, const float *__restrict__ rnorm,
                                                             const float *__restrict__ Wd, const float *__restrict__ Wu,
                                                             const float *__restrict__ bu, const float *__restrict__ gate, int M,
                                                             int G, float gate_T, float base, int self_kd, float *__restrict__ gx,
                                                             float *__restrict__ gh_out, float *__restrict__ sh_out,
                                                             double *__restrict__ part)
{
    __shared__ __align__(16) float gs[kMaxG * kD];
    __shared__ float ginv[kMaxG];
    __shared__ __align__(16) float scratch[kScratch];
    __shared__ float srow[kWaves][kWaveRows];
    __shared__ float coef[kWaves][kWaveRows][5];      // a, b (gx), alpha, beta (g_gate), w (g_b_up)
    __shared__ int idrow[kWaves][kWaveRows];
    __shared__ float bdp[kWaves][kH];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, hh = lane >> 5;
    const int row0 = (int)blockIdx.x * kPanel + wave * kWaveRows;
    const int row = row0 + r, rowc = row < M ? row : M - 1;
    float *tile = scratch + kOffTile + wave * kWaveRows * kHS, *dots = scratch + kOffDots + wave * kWaveRows * kPS;

    normalise_gate(gate, G, gs, ginv, wave, lane);
    const float sc_r = scale[rowc], c_r = cosv[rowc], rn_r = rnorm[rowc];
    const int id_r = amax[rowc];
    if (hh == 0) srow[wave][r] = sc_r;
    __syncthreads();

    // ---- t = grad_y W_u  [32, 64], and grad_y . b_u per row -------------------------------------------------------------------------
    f32x16 acc[2][2];
#pragma unroll
    for (int j = 0; j < 2; ++j) { acc[j][0] = zero16(); acc[j][1] = zero16(); }
    float gb = 0.f;
#pragma unroll
    for (int c = 0; c < kD / 64; ++c) {
        const int k0 = 64 * c + 32 * hh;
        float ga[32], bb[32];
        load_floats(gy + (size_t)rowc * kD + k0, ga);
        load_floats(bu + k0, bb);
        float gb_l = 0.f;
#pragma unroll
        for (int t = 0; t < 32; ++t) gb_l = fmaf(ga[t], bb[t], gb_l);
        gb += gb_l;
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int t = 0; t < 32; ++t)
                acc[j][c & 1] = __builtin_amdgcn_mfma_f32_32x32x2f32(ga[t], Wu[(size_t)(k0 + t) * kH + 32 * j + r], acc[j][c & 1], 0, 0, 0);
    }
    gb += xhalf(gb);

    // ---- gh, scale * h, the row dots' pieces, g_b_down ------------------------------------------------------------------------------
    float p[16], gbd[2];
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) p[reg] = 0.f;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int n = 32 * j + r;
        gbd[j] = 0.f;
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const int rl = rowmap(reg, hh), rw = row0 + rl;
            const bool valid = rw < M;
            const float hv = h[(size_t)(valid ? rw : M - 1) * kH + n];
            const float tv = acc[j][0][reg] + acc[j][1][reg], s = srow[wave][rl];
            const float ghv = hv > 0.f ? s * tv : 0.f;
            p[reg] = fmaf(tv, hv, p[reg]);
            tile[rl * kHS + n] = ghv;
            if (valid) {
                gh_out[(size_t)rw * kH + n] = ghv;
                sh_out[(size_t)rw * kH + n] = s * hv;
                gbd[j] += ghv;
            }
        }
    }
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) dots[rowmap(reg, hh) * kPS + r] = p[reg];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        gbd[j] += xhalf(gbd[j]);
        if (hh == 0) bdp[wave][32 * j + r] = gbd[j];
    }
    __syncthreads();

    // ---- per row: d loss / d scale, then the coefficients of the gate's path ----------------------------------------------------------
    {
        float dot = 0.f;
#pragma unroll
        for (int i = 0; i < 32; ++i) dot += dots[r * kPS + i];
        const float g_s = dot + gb;
        GateCoeffs co = {0.f, 0.f, 0.f, 0.f};
        if (G > 0) co = gate_backward_coeffs(g_s * gate_T * sc_r * (1.f - sc_r / base), c_r, rn_r, ginv[id_r]);
        if (hh == 0) {
            coef[wave][r][0] = co.a; coef[wave][r][1] = co.b; coef[wave][r][2] = co.alpha; coef[wave][r][3] = co.beta;
            coef[wave][r][4] = sc_r;
            idrow[wave][r] = G > 0 ? id_r : 0;
        }
    }
    float ga2[32];
#pragma unroll
    for (int t = 0; t < 32; ++t) ga2[t] = tile[r * kHS + 32 * hh + t];
    __syncthreads();

    // ---- gx = gh W_d + the gate's path + the L1 term's ------------------------------------------------------------------------------
    const float kd = (self_kd && grad_loss) ? grad_loss[0] / ((float)M * (float)kD) : 0.f;
#pragma unroll 1
    for (int jp = 0; jp < kD / 64; ++jp) {
        f32x16 o[2];
#pragma unroll
        for (int jj = 0; jj < 2; ++jj) {
            o[jj] = zero16();
            const int n = 64 * jp + 32 * jj + r;
#pragma unroll
            for (int t = 0; t < 32; ++t)
                o[jj] = __builtin_amdgcn_mfma_f32_32x32x2f32(ga2[t], Wd[(size_t)(32 * hh + t) * kD + n], o[jj], 0, 0, 0);
        }
#pragma unroll
        for (int jj = 0; jj < 2; ++jj) {
            const int n = 64 * jp + 32 * jj + r;
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const int rl = rowmap(reg, hh), rw = row0 + rl;
                if (rw < M) {
                    const float xv = x[(size_t)rw * kD + n];
                    float v = o[jj][reg];
                    if (G > 0) v += coef[wave][rl][0] * gs[idrow[wave][rl] * kD + n] + coef[wave][rl][1] * xv;
                    if (kd != 0.f) v += xv > 0.f ? kd : (xv < 0.f ? -kd : 0.f);
                    gx[(size_t)rw * kD + n] = v;
                }
            }
        }
    }

    // ---- the wave's rows once more, a row per step and four columns per lane: g_b_up and g_gate ---------------------------------------
    float4 gbu = make_float4(0.f, 0.f, 0.f, 0.f), gg[kMaxG];
#pragma unroll
    for (int g = 0; g < kMaxG; ++g) gg[g] = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int rr = 0; rr < kWaveRows && row0 + rr < M; ++rr) {
        const size_t o = (size_t)(row0 + rr) * kD + 4 * lane;
        const float4 gv = *reinterpret_cast<const float4 *>(gy + o);
        const float w = coef[wave][rr][4];
        gbu.x = fmaf(w, gv.x, gbu.x); gbu.y = fmaf(w, gv.y, gbu.y); gbu.z = fmaf(w, gv.z, gbu.z); gbu.w = fmaf(w, gv.w, gbu.w);
        if (G > 0) {
            const int id = __builtin_amdgcn_readfirstlane(idrow[wave][rr]);
            const float al = coef[wave][rr][2], be = coef[wave][rr][3];
            const float4 xv = *reinterpret_cast<const float4 *>(x + o);
            const float4 gh4 = *reinterpret_cast<const float4 *>(gs + id * kD + 4 * lane);
            const float4 d = make_float4(fmaf(al, xv.x, be * gh4.x), fmaf(al, xv.y, be * gh4.y), fmaf(al, xv.z, be * gh4.z),
                                         fmaf(al, xv.w, be * gh4.w));
#pragma unroll
            for (int g = 0; g < kMaxG; ++g)
                if (id == g) { gg[g].x += d.x; gg[g].y += d.y; gg[g].z += d.z; gg[g].w += d.w; }
        }
    }
    __syncthreads();      // (every wave is done with its tile and its row dots: the sums move through the same words)
    float *wp = scratch + wave * kWavePart;
    *reinterpret_cast<float4 *>(wp + 4 * lane) = gbu;
#pragma unroll
    for (int g = 0; g < kMaxG; ++g) *reinterpret_cast<float4 *>(wp + kD + g * kD + 4 * lane) = gg[g];
    __syncthreads();
    double *mine = part + (size_t)blockIdx.x * kBwdPart;
    if (tid < kH) mine[tid] = (((double)bdp[0][tid] + (double)bdp[1][tid]) + (double)bdp[2][tid]) + (double)bdp[3][tid];
    for (int e = tid; e < kWavePart; e += kThreads)
        mine[kH + e] = (((double)scratch[e] + (double)scratch[kWavePart + e]) + (double)scratch[2 * kWavePart + e])
                       + (double)scratch[3 * kWavePart + e];
}

// (the structure of cet_bwd_fold; one kernel template for both came out as other machine code)
// out element e < n_out: the sum over the blocks' doubles in index order.  A block folds 16 elements: 16 groups of threads each
// add every 16th block's partial, LDS joins the groups in a fixed order.  e: [0, 64) g_b_down, [64, 320) g_b_up, the rest g_gate.
__global__ __launch_bounds__(kThreads) void adapter_bwd_fold(const double *__restrict__ part, int nblocks, int n_out,
                                                             float *__restrict__ g_bd, float *__restrict__ g_bu,
                                                             float *__restrict__ g_gate)
{
    __shared__ double red[16][16];
    const int o = threadIdx.x % 16, cg = threadIdx.x / 16, e = (int)blockIdx.x * 16 + o;
    double s = 0.0;
    if (e < n_out)
        for (int b = cg; b < nblocks; b += 16) s += part[(size_t)b * kBwdPart + e];
    red[cg][o] = s;
    __syncthreads();
    if (cg == 0 && e < n_out) {
        for (int g = 1; g < 16; ++g) s += red[g][o];
        if (e < kH) g_bd[e] = (float)s;
        else if (e < kH + kD) g_bu[e - kH] = (float)s;
        else g_gate[e - kH - kD] = (float)s;
    }
}

inline size_t blocks_of(long long M) { return (size_t)((M + kPanel - 1) / kPanel); }

// workspace (floats): [the blocks' doubles: max(1, kBwdPart) per block][gh M x 64][scale * h M x 64][zira_xty_f32's scratch]
struct Layout {
    size_t part, gh, sh, xty, total;
};
inline Layout layout(long long M)
{
    Layout l;
    l.part = 0;
    l.gh = align4(2 * blocks_of(M) * kBwdPart);
    l.sh = l.gh + (size_t)M * kH;
    l.xty = l.sh + (size_t)M * kH;
    l.total = l.xty + align4(zira::max_xty_workspace(M, {{kH, kD}, {kD, kH}}));
    return l;
}

}  // namespace

extern "C" {

size_t zira_adapter_workspace_floats(long long M, int D, int H)
{
    if (D != kD || H != kH || M < 1 || M > kMaxM) return 0;
    return layout(M).total;
}

int zira_adapter_fwd_f32(const float *x, const float *w_down, const float *b_down, const float *w_up, const float *b_up,
                         const float *gate, long long M, int G, float gate_T, float gate_base_scale, int self_kd, float *y,
                         float *loss, float *h, float *scale, int32_t *amax, float *cosv, float *rnorm, float *workspace,
                         uint32_t *counter, void *stream)
{
    if (M < 1 || M > kMaxM || G < 0 || G > kMaxG || (G > 0) != (gate != nullptr)) return -1;
    if (!x || !w_down || !b_down || !w_up || !b_up || !y || !loss || !h || !scale || !amax || !cosv || !rnorm || !workspace) return -1;
    if (self_kd && !counter) return -1;
    if (misaligned(x) || misaligned(w_down) || misaligned(b_down) || misaligned(w_up) || misaligned(b_up) || misaligned(gate)
        || misaligned(y) || misaligned(h) || misaligned(workspace)) return -1;
    hipLaunchKernelGGL(adapter_fwd, dim3((unsigned)blocks_of(M)), dim3(kThreads), 0, (hipStream_t)stream, x, w_down, b_down, w_up,
                       b_up, gate, (int)M, G, gate_T, gate_base_scale, self_kd, y, loss, h, scale, amax, cosv, rnorm,
                       reinterpret_cast<double *>(workspace), counter);
    return (int)hipGetLastError();
}

int zira_adapter_bwd_f32(const float *grad_y, const float *grad_loss, const float *x, const float *h, const float *scale,
                         const int32_t *amax, const float *cosv, const float *rnorm, const float *w_down, const float *w_up,
                         const float *b_up, const float *gate, long long M, int G, float gate_T, float gate_base_scale,
                         int self_kd, float *gx, float *g_w_down, float *g_b_down, float *g_w_up, float *g_b_up, float *g_gate,
                         float *workspace, void *stream)
{
    if (M < 1 || M > kMaxM || G < 0 || G > kMaxG || (G > 0) != (gate != nullptr) || (G > 0) != (g_gate != nullptr)) return -1;
    if (!grad_y || !x || !h || !scale || !amax || !cosv || !rnorm || !w_down || !w_up || !b_up || !gx || !g_w_down || !g_b_down
        || !g_w_up || !g_b_up || !workspace) return -1;
    if (misaligned(grad_y) || misaligned(x) || misaligned(h) || misaligned(w_down) || misaligned(w_up) || misaligned(b_up)
        || misaligned(gate) || misaligned(gx) || misaligned(g_w_down) || misaligned(g_w_up) || misaligned(workspace)) return -1;
    const Layout l = layout(M);
    const int nblocks = (int)blocks_of(M), n_out = kH + kD + G * kD;
    double *part = reinterpret_cast<double *>(workspace + l.part);
    float *gh = workspace + l.gh, *sh = workspace + l.sh, *xws = workspace + l.xty;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(adapter_bwd_rows, dim3((unsigned)nblocks), dim3(kThreads), 0, st, grad_y, grad_loss, x, h, scale, amax, cosv,
                       rnorm, w_down, w_up, b_up, gate, (int)M, G, gate_T, gate_base_scale, self_kd, gx, gh, sh, part);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(adapter_bwd_fold, dim3((unsigned)((n_out + 15) / 16)), dim3(kThreads), 0, st, part, nblocks, n_out, g_b_down,
                       g_b_up, g_gate);
    e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    int rc = zira_xty_f32(gh, x, 1, (int)M, kH, kD, 0, g_w_down, xws, stream);          // g_W_down [64, 256] = gh^T x
    if (rc != 0) return rc;
    return zira_xty_f32(grad_y, sh, 1, (int)M, kD, kH, 0, g_w_up, xws, stream);         // g_W_up [256, 64] = grad_y^T (scale * h)
}

}  // extern "C"
