// place.hip -- a minibatch of differently sized images into one fixed canvas, as ONE launch: the normalised batch tensor
// [B, 3, Hc, Wc] (fp32, (x - mean[c]) / std[c] inside image b's rectangle, zero elsewhere) and the padding mask [B, Hc, Wc]
// (bool, true outside the rectangle).  Every output element is written exactly once -- no fill in front of the launch -- and
// the arithmetic is the op chain's: convert to fp32, one subtract, one correctly rounded IEEE divide (no reciprocal, no
// contraction possible), so the canvas holds the bits of `(x.float() - mean) / std`.
//
// The sources are separate allocations.  Their pointers, sizes and strides travel BY VALUE in the kernel's argument struct (up
// to 8 images, 32 bytes each): nothing is uploaded and the host never waits, so the launch can be captured.
//
// Work: a thread owns four neighbouring pixels of one canvas row in all three channels: three 16-byte stores to the canvas,
// one 4-byte store (four bools) to the mask.  blockIdx.y is the image, so the image's descriptor is read with scalar loads.
// The canvas is 16-byte aligned by construction (Wc % 4 == 0, checked at the entry); a source row starts wherever h, w and
// the allocation put it, so a group that lies inside the image is read with one load typed to the ELEMENT's alignment (16
// bytes dword-aligned for fp32, 4 bytes at any address for uint8: gfx950's global loads need no more) and the tail group of
// a row whose width is no multiple of four element by element.  A canvas whose width is no multiple of four, or whose base is
// unaligned, takes the one-pixel form of the same kernel.
//
// Bound: a streaming copy -- each source byte read once, each canvas / mask byte written once:
//   sum_i 3 h_i w_i sizeof(T)  +  B Hc Wc (3 * 4 + 1) bytes.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "zira_msda.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxImages = ZIRA_PLACE_MAX_IMAGES;

struct PlaceArgs {
    zira_place_image img[kMaxImages];
    float mean[3];
    float stdev[3];
    float *canvas;
    unsigned char *mask;
    int n_images, Hc, Wc;
};

__device__ __forceinline__ float to_f32(float v) { return v; }
__device__ __forceinline__ float to_f32(unsigned char v) { return (float)v; }

typedef float f4 __attribute__((ext_vector_type(4), aligned(4)));   // 16 bytes, dword aligned
typedef uint32_t u32_any __attribute__((aligned(1)));               // 4 bytes at any address

// four neighbouring source elements in one load: the address needs the element type's alignment only
__device__ __forceinline__ void load4(const float *p, float (&v)[4])
{
    const f4 q = *reinterpret_cast<const f4 *>(p);
    v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
}
__device__ __forceinline__ void load4(const unsigned char *p, float (&v)[4])
{
    const uint32_t q = *reinterpret_cast<const u32_any *>(p);
    v[0] = (float)(q & 255u), v[1] = (float)((q >> 8) & 255u), v[2] = (float)((q >> 16) & 255u), v[3] = (float)(q >> 24);
}

// (x - mean) / stdev where keep, +0.0 elsewhere -- as a mask on the bits, so that the divide stays straight-line code
__device__ __forceinline__ float normalised(float x, float mean, float stdev, bool keep)
{
    return __int_as_float(__float_as_int((x - mean) / stdev) & -(int)keep);
}

template <typename T, int VEC>
__global__ __launch_bounds__(kThreads) void place_kernel(const PlaceArgs a)
{
    const int b = blockIdx.y;                          // wave-uniform: the descriptor comes through scalar loads
    const int groups_per_row = a.Wc / VEC;
    const long long t = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (t >= (long long)a.Hc * groups_per_row) return;
    const int y = (int)(t / groups_per_row);
    const int x = (int)(t - (long long)y * groups_per_row) * VEC;

    const zira_place_image im = a.img[b];
    const int n_in = (y < im.h) ? min(max(im.w - x, 0), VEC) : 0;    // pixels of this group inside the image
    const T *src = static_cast<const T *>(im.data) + (long long)y * im.stride_r + x;

    float v[3][VEC];
    if (VEC == 4 && n_in == 4) {                       // the body of a row: one load per channel
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float w4[4];
            load4(src + c * im.stride_c, w4);
#pragma unroll
            for (int j = 0; j < VEC; ++j) v[c][j] = w4[j % 4];
        }
    } else {                                           // a row's tail group, the padding, the one-pixel form
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int j = 0; j < VEC; ++j) v[c][j] = (j < n_in) ? to_f32(src[c * im.stride_c + j]) : 0.0f;
    }

    const long long plane = (long long)a.Hc * a.Wc;
    const long long pix = (long long)y * a.Wc + x;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float o[VEC];
#pragma unroll
        for (int j = 0; j < VEC; ++j) o[j] = normalised(v[c][j], a.mean[c], a.stdev[c], j < n_in);
        float *dst = a.canvas + ((long long)b * 3 + c) * plane + pix;
        if constexpr (VEC == 4) *reinterpret_cast<float4 *>(dst) = make_float4(o[0], o[1], o[2], o[3]);
        else dst[0] = o[0];
    }
    unsigned char *m = a.mask + (long long)b * plane + pix;
    if constexpr (VEC == 4) {
        uint32_t bits = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) bits |= (uint32_t)(j >= n_in) << (8 * j);
        *reinterpret_cast<uint32_t *>(m) = bits;
    } else {
        m[0] = (unsigned char)(n_in == 0);
    }
}

template <typename T>
int place_batch(const zira_place_image *images, int n_images, int Hc, int Wc, const float (&mean)[3], const float (&stdev)[3],
                float *canvas, unsigned char *mask, void *stream)
{
    if (!images || !canvas || !mask || n_images < 1 || n_images > kMaxImages) return ZIRA_MSDA_EINVAL;
    if (Hc < 1 || Wc < 1 || (long long)Hc * Wc > (1ll << 30)) return ZIRA_MSDA_EINVAL;
    if (reinterpret_cast<uintptr_t>(canvas) & 3) return ZIRA_MSDA_EINVAL;
    PlaceArgs a = {};
    for (int i = 0; i < n_images; ++i) {
        const zira_place_image &im = images[i];
        // the image fits the canvas, rows and channel planes do not overlap, the element type's alignment holds
        if (!im.data || im.h < 1 || im.w < 1 || im.h > Hc || im.w > Wc) return ZIRA_MSDA_EINVAL;
        if (im.stride_r < im.w || im.stride_c < (int64_t)im.h * im.stride_r - (im.stride_r - im.w)) return ZIRA_MSDA_EINVAL;
        if (reinterpret_cast<uintptr_t>(im.data) & (sizeof(T) - 1)) return ZIRA_MSDA_EINVAL;
        a.img[i] = im;
    }
    for (int c = 0; c < 3; ++c) a.mean[c] = mean[c], a.stdev[c] = stdev[c];
    a.canvas = canvas, a.mask = mask, a.n_images = n_images, a.Hc = Hc, a.Wc = Wc;
    const bool vec = Wc % 4 == 0 && (reinterpret_cast<uintptr_t>(canvas) & 15) == 0 && (reinterpret_cast<uintptr_t>(mask) & 3) == 0;
    const long long groups = (long long)Hc * (vec ? Wc / 4 : Wc);
    const dim3 grid((unsigned)((groups + kThreads - 1) / kThreads), (unsigned)n_images);
    if (vec) hipLaunchKernelGGL((place_kernel<T, 4>), grid, dim3(kThreads), 0, static_cast<hipStream_t>(stream), a);
    else hipLaunchKernelGGL((place_kernel<T, 1>), grid, dim3(kThreads), 0, static_cast<hipStream_t>(stream), a);
    return (int)hipGetLastError();
}

}  // namespace

extern "C" int zira_place_batch_f32(const zira_place_image *images, int n_images, int Hc, int Wc, float mean0, float mean1,
                                    float mean2, float std0, float std1, float std2, float *canvas, unsigned char *mask,
                                    void *stream)
{
    const float mean[3] = {mean0, mean1, mean2}, stdev[3] = {std0, std1, std2};
    return place_batch<float>(images, n_images, Hc, Wc, mean, stdev, canvas, mask, stream);
}

extern "C" int zira_place_batch_u8(const zira_place_image *images, int n_images, int Hc, int Wc, float mean0, float mean1,
                                   float mean2, float std0, float std1, float std2, float *canvas, unsigned char *mask,
                                   void *stream)
{
    const float mean[3] = {mean0, mean1, mean2}, stdev[3] = {std0, std1, std2};
    return place_batch<unsigned char>(images, n_images, Hc, Wc, mean, stdev, canvas, mask, stream);
}
