// resample.hip -- Pillow's bilinear `Image.resize` of uint8 images on the device, bit for bit, for a minibatch of up to 8
// images of different sizes: what detectron2's ResizeTransform computes for the reference's data mapper.
//
// The arithmetic, per axis with input length `in` and output length `out` (all of it float64, every operation rounded on its
// own -- the file is compiled with -ffp-contract=off, and the fp64 divides are the correctly rounded ones):
//   scale = in / out, fs = max(scale, 1), support = fs, ss = 1 / fs
//   center = (xx + 0.5) scale, xmin = max(trunc(center - support + 0.5), 0), xmax = min(trunc(center + support + 0.5), in) - xmin
//   w[x] = 1 - a where a = |(x + xmin - center + 0.5) ss| < 1, else 0;  ww = sum of w[x] in index order;  w[x] /= ww
//   k[x] = trunc(w[x] 2^22 + 0.5)
//   one pass: clamp((2^21 + sum pixel k) >> 22, 0, 255) in integers
// The horizontal pass runs first and produces a uint8 image, the vertical pass reads that.  An axis with out == in is not
// special here: its taps come out as (2^22, 0) and the pass reproduces the bytes.
//
// zira_resample_coeffs: one thread per output index of one (image, axis) writes (xmin, xmax) and ksize int32 taps (the unused
//   ones zero) into the workspace.  The weights are computed twice -- once for ww, once for the taps -- instead of being kept
//   in a runtime-indexed array.
// zira_resample_u8: a block owns a 16 x 64 tile of one image's output in all three channels.  It reads its slice of both tap
//   tables into LDS once, then walks the source rows its tile needs, 8 at a time: the rows' needed column range (all channels)
//   into LDS, the horizontal pass out of LDS into the uint8 intermediate (LDS, 64 bytes per row and channel), and at the end
//   the vertical pass out of LDS, four neighbouring pixels per thread, stored as one dword where all four exist and byte by byte
//   in a row's tail.  Every output byte is written once; no fill, no atomics.
// Both: sizes, strides, pointers and table offsets travel BY VALUE in the kernel's argument struct; nothing is uploaded and the
// host never waits, so the launches can be captured.
//
// Bound: a streaming pass -- source bytes read once plus the halo between tiles (2 support rows per 16-row tile, 2 support
// columns per 64-column tile), output bytes written once:  sum_i 3 (h_i w_i + new_h_i new_w_i) bytes plus the tables.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "zira_msda.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxImages = ZIRA_RESAMPLE_MAX_IMAGES;
constexpr int kMaxSide = ZIRA_RESAMPLE_MAX_SIDE;
constexpr int kMaxTaps = ZIRA_RESAMPLE_MAX_TAPS;
constexpr int kBits = 22;

constexpr int kTileH = 16, kTileW = 64;
constexpr int kStageRows = 8;
// source columns one tile can need: (kTileW - 1) scale + 2 support + 1 at scale = support = 8, rounded up
constexpr int kStageCols = 528;
// intermediate rows one tile can need: (kTileH - 1) scale + 2 support + 1 at scale = support = 8, rounded up
constexpr int kInterRows = 140;
static_assert((kTileW - 1) * 8 + 17 <= kStageCols && (kTileH - 1) * 8 + 17 <= kInterRows, "tile halo");

struct Axis {
    int32_t n_in, n_out, ksize;
    int32_t bounds, taps;        // offsets into the workspace, in int32 elements
};

struct Image {
    const unsigned char *src;
    unsigned char *dst;
    int64_t stride_c, stride_r, stride_x;
    int32_t flip;
    Axis ax[2];                  // 0: horizontal (w -> new_w), 1: vertical (h -> new_h)
};

struct Args {
    Image img[kMaxImages];
    int32_t *ws;
    int n_images;
};

int ksize_of(int n_in, int n_out)
{
    // ceil(max(in / out, 1)) * 2 + 1: the quotient of two lengths <= 4096 is an integer or at least 2^-12 away from one, so
    // the integer ceiling is the floating one
    return (n_in <= n_out ? 1 : (n_in + n_out - 1) / n_out) * 2 + 1;
}

// Fills the by-value struct; false where the call is not served.  `total` = int32 elements of workspace.
bool layout(const zira_resample_image *images, int n_images, Args &a, size_t &total)
{
    total = 0;
    if (!images || n_images < 1 || n_images > kMaxImages) return false;
    a.n_images = n_images;
    for (int i = 0; i < n_images; ++i) {
        const zira_resample_image &im = images[i];
        const int n_in[2] = {im.w, im.h}, n_out[2] = {im.new_w, im.new_h};
        for (int x = 0; x < 2; ++x) {
            if (n_in[x] < 1 || n_in[x] > kMaxSide || n_out[x] < 1 || n_out[x] > kMaxSide) return false;
            if ((int64_t)n_in[x] > 8 * (int64_t)n_out[x]) return false;         // downscale <= 8: ksize <= 17
            Axis &ax = a.img[i].ax[x];
            ax.n_in = n_in[x], ax.n_out = n_out[x], ax.ksize = ksize_of(n_in[x], n_out[x]);
            ax.bounds = (int32_t)total, total += 2 * (size_t)n_out[x];
            ax.taps = (int32_t)total, total += (size_t)ax.ksize * n_out[x];
        }
        a.img[i].src = static_cast<const unsigned char *>(im.src);
        a.img[i].dst = static_cast<unsigned char *>(im.dst);
        a.img[i].stride_c = im.stride_c, a.img[i].stride_r = im.stride_r, a.img[i].stride_x = im.stride_x;
        a.img[i].flip = im.flip != 0;
    }
    return true;
}

__device__ __forceinline__ double weight(int x, double center, double ss)
{
    double a = ((double)x - center + 0.5) * ss;
    if (a < 0.0) a = -a;
    return a < 1.0 ? 1.0 - a : 0.0;
}

__global__ __launch_bounds__(kThreads) void coeffs_kernel(const Args a)
{
    const Axis ax = a.img[blockIdx.y >> 1].ax[blockIdx.y & 1];
    const int xx = blockIdx.x * kThreads + threadIdx.x;
    if (xx >= ax.n_out) return;
    const double scale = (double)ax.n_in / (double)ax.n_out;
    const double fs = scale < 1.0 ? 1.0 : scale;
    const double support = fs;
    const double ss = 1.0 / fs;
    const double center = ((double)xx + 0.5) * scale;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > ax.n_in) xmax = ax.n_in;
    xmax -= xmin;
    if (xmax > ax.ksize) xmax = ax.ksize;      // never taken: ksize = 2 ceil(support) + 1 holds every window
    double ww = 0.0;
    for (int x = 0; x < xmax; ++x) ww += weight(x + xmin, center, ss);
    int32_t *k = a.ws + ax.taps + (int64_t)xx * ax.ksize;
    for (int x = 0; x < ax.ksize; ++x) {
        int32_t tap = 0;
        if (x < xmax) {
            double w = weight(x + xmin, center, ss);
            if (ww != 0.0) w /= ww;
            tap = w < 0.0 ? (int32_t)(-0.5 + w * (double)(1 << kBits)) : (int32_t)(0.5 + w * (double)(1 << kBits));
        }
        k[x] = tap;
    }
    a.ws[ax.bounds + 2 * xx] = xmin;
    a.ws[ax.bounds + 2 * xx + 1] = xmax;
}

__device__ __forceinline__ int clip8(int acc)
{
    return min(max(acc >> kBits, 0), 255);
}

typedef uint32_t u32_any __attribute__((aligned(1)));               // 4 bytes at any address

__global__ __launch_bounds__(kThreads) void resample_kernel(const Args a)
{
    __shared__ int32_t s_kh[kTileW * kMaxTaps];
    __shared__ int32_t s_kv[kTileH * kMaxTaps];
    __shared__ int32_t s_bh[kTileW * 2];
    __shared__ int32_t s_bv[kTileH * 2];
    __shared__ unsigned char s_stage[kStageRows * 3 * kStageCols];
    __shared__ uint32_t s_inter[kInterRows * 3 * (kTileW / 4)];      // bytes [row][channel][kTileW]

    const Image im = a.img[blockIdx.y];                // wave-uniform: the descriptor comes through scalar loads
    const Axis axh = im.ax[0], axv = im.ax[1];
    const int tiles_x = (axh.n_out + kTileW - 1) / kTileW;
    const int tiles_y = (axv.n_out + kTileH - 1) / kTileH;
    if ((int)blockIdx.x >= tiles_x * tiles_y) return;  // the grid is sized for the largest image of the batch
    const int ox0 = ((int)blockIdx.x % tiles_x) * kTileW, oy0 = ((int)blockIdx.x / tiles_x) * kTileH;
    const int tw = min(kTileW, axh.n_out - ox0), th = min(kTileH, axv.n_out - oy0);
    const int tid = threadIdx.x;

    // this tile's slice of both tables, once.  The bounds are clamped to the source whatever the workspace holds.
    for (int i = tid; i < tw; i += kThreads) {
        const int xmin = min(max(a.ws[axh.bounds + 2 * (ox0 + i)], 0), axh.n_in - 1);
        s_bh[2 * i] = xmin;
        s_bh[2 * i + 1] = min(max(a.ws[axh.bounds + 2 * (ox0 + i) + 1], 0), min(axh.ksize, axh.n_in - xmin));
    }
    for (int i = tid; i < th; i += kThreads) {
        const int ymin = min(max(a.ws[axv.bounds + 2 * (oy0 + i)], 0), axv.n_in - 1);
        s_bv[2 * i] = ymin;
        s_bv[2 * i + 1] = min(max(a.ws[axv.bounds + 2 * (oy0 + i) + 1], 0), min(axv.ksize, axv.n_in - ymin));
    }
    for (int i = tid; i < tw * axh.ksize; i += kThreads) s_kh[i] = a.ws[axh.taps + (int64_t)ox0 * axh.ksize + i];
    for (int i = tid; i < th * axv.ksize; i += kThreads) s_kv[i] = a.ws[axv.taps + (int64_t)oy0 * axv.ksize + i];
    __syncthreads();

    // the source window of the tile: columns [c0, c0 + ncols), rows [r0, r0 + nrows)
    int c0 = s_bh[0], c1 = s_bh[0] + s_bh[1];
    for (int i = 1; i < tw; ++i) c0 = min(c0, s_bh[2 * i]), c1 = max(c1, s_bh[2 * i] + s_bh[2 * i + 1]);
    int r0 = s_bv[0], r1 = s_bv[0] + s_bv[1];
    for (int i = 1; i < th; ++i) r0 = min(r0, s_bv[2 * i]), r1 = max(r1, s_bv[2 * i] + s_bv[2 * i + 1]);
    const int ncols = min(c1 - c0, kStageCols), nrows = min(r1 - r0, kInterRows);
    const bool pixel_major = im.stride_c < im.stride_x;             // HWC: the channels of a pixel are neighbours in memory

    unsigned char *inter = reinterpret_cast<unsigned char *>(s_inter);
    for (int rb = 0; rb < nrows; rb += kStageRows) {
        const int nr = min(kStageRows, nrows - rb);
        // the rows' window into LDS, neighbouring lanes on neighbouring bytes of the source
        const int per_row = 3 * ncols;
        for (int i = tid; i < nr * per_row; i += kThreads) {
            const int rr = i / per_row, e = i - rr * per_row;
            const int c = pixel_major ? e % 3 : e / ncols, j = pixel_major ? e / 3 : e - c * ncols;
            const int x = im.flip ? axh.n_in - 1 - (c0 + j) : c0 + j;
            s_stage[(rr * 3 + c) * kStageCols + j] =
                im.src[c * im.stride_c + (int64_t)(r0 + rb + rr) * im.stride_r + x * im.stride_x];
        }
        __syncthreads();
        // horizontal pass: uint8 intermediate
        for (int i = tid; i < nr * 3 * kTileW; i += kThreads) {
            const int ox = i % kTileW, rc = i / kTileW;             // rc = rr * 3 + c
            if (ox >= tw) continue;
            const int j0 = s_bh[2 * ox] - c0, n = min(s_bh[2 * ox + 1], ncols - j0);
            const unsigned char *row = s_stage + rc * kStageCols + j0;
            const int32_t *k = s_kh + ox * axh.ksize;
            int acc = 1 << (kBits - 1);
            for (int x = 0; x < n; ++x) acc += (int)row[x] * k[x];
            inter[(rb * 3 + rc) * kTileW + ox] = (unsigned char)clip8(acc);
        }
        __syncthreads();
    }

    // vertical pass: four neighbouring pixels of one output row and channel per thread
    constexpr int kGroups = kTileW / 4;
    for (int i = tid; i < th * 3 * kGroups; i += kThreads) {
        const int g = i % kGroups, c = (i / kGroups) % 3, oy = i / (3 * kGroups);
        const int ox = 4 * g;
        if (ox >= tw) continue;
        const int y0 = s_bv[2 * oy] - r0, n = min(s_bv[2 * oy + 1], nrows - y0);
        const int32_t *k = s_kv + oy * axv.ksize;
        int acc[4] = {1 << (kBits - 1), 1 << (kBits - 1), 1 << (kBits - 1), 1 << (kBits - 1)};
        for (int y = 0; y < n; ++y) {
            const uint32_t q = s_inter[((y0 + y) * 3 + c) * kGroups + g];
            const int kk = k[y];
            acc[0] += (int)(q & 255u) * kk, acc[1] += (int)((q >> 8) & 255u) * kk;
            acc[2] += (int)((q >> 16) & 255u) * kk, acc[3] += (int)(q >> 24) * kk;
        }
        unsigned char *dst = im.dst + ((int64_t)c * axv.n_out + (oy0 + oy)) * axh.n_out + ox0 + ox;
        if (ox + 4 <= tw) {
            *reinterpret_cast<u32_any *>(dst) = (uint32_t)clip8(acc[0]) | ((uint32_t)clip8(acc[1]) << 8) |
                                                ((uint32_t)clip8(acc[2]) << 16) | ((uint32_t)clip8(acc[3]) << 24);
        } else {
            for (int j = 0; j < tw - ox; ++j) dst[j] = (unsigned char)clip8(acc[j]);
        }
    }
}

}  // namespace

extern "C" size_t zira_resample_ws_bytes(const zira_resample_image *images, int n_images)
{
    Args a = {};
    size_t total = 0;
    if (!layout(images, n_images, a, total)) return 0;
    return total * sizeof(int32_t);
}

extern "C" int zira_resample_coeffs(const zira_resample_image *images, int n_images, void *ws, size_t ws_bytes, void *stream)
{
    Args a = {};
    size_t total = 0;
    if (!layout(images, n_images, a, total)) return ZIRA_MSDA_EINVAL;
    if (!ws || ws_bytes < total * sizeof(int32_t) || (reinterpret_cast<uintptr_t>(ws) & 3)) return ZIRA_MSDA_EINVAL;
    a.ws = static_cast<int32_t *>(ws);
    int longest = 1;
    for (int i = 0; i < n_images; ++i) longest = max(longest, max(a.img[i].ax[0].n_out, a.img[i].ax[1].n_out));
    const dim3 grid((unsigned)((longest + kThreads - 1) / kThreads), (unsigned)(2 * n_images));
    hipLaunchKernelGGL(coeffs_kernel, grid, dim3(kThreads), 0, static_cast<hipStream_t>(stream), a);
    return (int)hipGetLastError();
}

extern "C" int zira_resample_u8(const zira_resample_image *images, int n_images, const void *ws, size_t ws_bytes, void *stream)
{
    Args a = {};
    size_t total = 0;
    if (!layout(images, n_images, a, total)) return ZIRA_MSDA_EINVAL;
    if (!ws || ws_bytes < total * sizeof(int32_t) || (reinterpret_cast<uintptr_t>(ws) & 3)) return ZIRA_MSDA_EINVAL;
    int tiles = 1;
    for (int i = 0; i < n_images; ++i) {
        const Image &im = a.img[i];
        if (!im.src || !im.dst || im.stride_c < 1 || im.stride_r < 1 || im.stride_x < 1) return ZIRA_MSDA_EINVAL;
        tiles = max(tiles, ((im.ax[0].n_out + kTileW - 1) / kTileW) * ((im.ax[1].n_out + kTileH - 1) / kTileH));
    }
    a.ws = const_cast<int32_t *>(static_cast<const int32_t *>(ws));
    hipLaunchKernelGGL(resample_kernel, dim3((unsigned)tiles, (unsigned)n_images), dim3(kThreads), 0,
                       static_cast<hipStream_t>(stream), a);
    return (int)hipGetLastError();
}
