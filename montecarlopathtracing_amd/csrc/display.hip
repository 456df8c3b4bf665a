// The display transform on the GPU (mcpt.h: display transform): the luminance histogram of a linear fp64 frame and its map to 8-bit
// pixels.  The arithmetic is display_math.hpp's, shared with mcpt_display_host; tests/display_ref.py restates it in numpy.  The histogram
// counts integers, so its result is exact and independent of the grid and of the order of the adds; the map forms every byte in one lane.
#include <hip/hip_runtime.h>

#include "display.hpp"

namespace mcpt {

static constexpr int kDisplayBlock = 256;
static constexpr unsigned kHistogramMaxBlocks = 1024;      // a block counts at most ceil(n / 1024) + 256 pixels: far below 2^32 for any frame

// ---- histogram: blocks of 256 lanes stride over the listed pixels.  Each block counts into a uint32 histogram in LDS (LDS atomics; a
// frame of one value sends every lane to one slot, which only serialises them) and adds its non-zero slots to the global counts with
// device-scope 64-bit atomics: blocks on different XCDs add to the same words.
__global__ void __launch_bounds__(kDisplayBlock) k_display_histogram(const double* __restrict__ img, const int32_t* __restrict__ pixels, long long n,
                                                                     unsigned long long* __restrict__ slots)
{
    __shared__ unsigned int h[MCPT_DISPLAY_SLOTS];
    for (int s = threadIdx.x; s < MCPT_DISPLAY_SLOTS; s += kDisplayBlock) h[s] = 0u;
    __syncthreads();
    const long long stride = (long long)gridDim.x * kDisplayBlock;
    for (long long i = (long long)blockIdx.x * kDisplayBlock + threadIdx.x; i < n; i += stride) {
        const size_t pix = pixels ? (size_t)pixels[i] : (size_t)i;
        const double* c = img + pix * 3;
        atomicAdd(&h[display_slot(display_luminance(c[0], c[1], c[2]))], 1u);
    }
    __syncthreads();
    for (int s = threadIdx.x; s < MCPT_DISPLAY_SLOTS; s += kDisplayBlock) {
        const unsigned int v = h[s];
        if (v != 0u) __hip_atomic_fetch_add(&slots[s], (unsigned long long)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// ---- map, the whole frame: lane i maps pixels 4 i .. 4 i + 3 -- 96 bytes of the frame in six 16-byte loads -- and writes their 12 bytes
// as three dwords (RGBA: their 16 bytes as one 16-byte store).  The lane after the last full one maps the 1 to 3 pixels left, byte by byte.
template <bool RGBA>
__global__ void __launch_bounds__(kDisplayBlock) k_display_map(const double* __restrict__ img, long long n, DisplayMap m, uint8_t* __restrict__ out)
{
    const long long i = (long long)blockIdx.x * kDisplayBlock + threadIdx.x;
    const long long full = n >> 2;
    if (i < full) {
        const double2* src = reinterpret_cast<const double2*>(img) + i * 6;
        double c[12];
        for (int k = 0; k < 6; k++) { const double2 v = src[k]; c[2 * k] = v.x; c[2 * k + 1] = v.y; }
        uint8_t b[12];
        for (int p = 0; p < 4; p++) display_pixel(m, c + 3 * p, b + 3 * p);
        if constexpr (RGBA) {
            uint4 w;
            w.x = b[0] | (b[1] << 8) | (b[2] << 16) | 0xff000000u;
            w.y = b[3] | (b[4] << 8) | (b[5] << 16) | 0xff000000u;
            w.z = b[6] | (b[7] << 8) | (b[8] << 16) | 0xff000000u;
            w.w = b[9] | (b[10] << 8) | (b[11] << 16) | 0xff000000u;
            reinterpret_cast<uint4*>(out)[i] = w;
        } else {
            unsigned int* dst = reinterpret_cast<unsigned int*>(out) + i * 3;
            for (int k = 0; k < 3; k++)
                dst[k] = b[4 * k] | (b[4 * k + 1] << 8) | (b[4 * k + 2] << 16) | ((unsigned int)b[4 * k + 3] << 24);
        }
        return;
    }
    if (i != full) return;
    constexpr int kBytes = RGBA ? 4 : 3;
    for (long long pix = full << 2; pix < n; pix++) {
        const double c[3] = {img[pix * 3], img[pix * 3 + 1], img[pix * 3 + 2]};
        uint8_t b[3];
        display_pixel(m, c, b);
        uint8_t* dst = out + pix * kBytes;
        dst[0] = b[0]; dst[1] = b[1]; dst[2] = b[2];
        if constexpr (RGBA) dst[3] = 255;
    }
}

// ---- map, a pixel list (or a frame whose pointers are not aligned for the above): one lane per pixel, byte stores at the pixel's own
// place; nothing else is written.
template <bool RGBA>
__global__ void __launch_bounds__(kDisplayBlock) k_display_map_list(const double* __restrict__ img, const int32_t* __restrict__ pixels, long long n,
                                                                    DisplayMap m, uint8_t* __restrict__ out)
{
    const long long i = (long long)blockIdx.x * kDisplayBlock + threadIdx.x;
    if (i >= n) return;
    const size_t pix = pixels ? (size_t)pixels[i] : (size_t)i;
    const double c[3] = {img[pix * 3], img[pix * 3 + 1], img[pix * 3 + 2]};
    uint8_t b[3];
    display_pixel(m, c, b);
    uint8_t* dst = out + pix * (RGBA ? 4 : 3);
    dst[0] = b[0]; dst[1] = b[1]; dst[2] = b[2];
    if constexpr (RGBA) dst[3] = 255;
}

static inline unsigned blocks_of(long long n) { return (unsigned)((n + kDisplayBlock - 1) / kDisplayBlock); }

void launch_display_histogram(const double* d_img, const int32_t* d_pixels, long long n, unsigned long long* d_slots, hipStream_t st)
{
    if (n <= 0) return;
    const unsigned blocks = blocks_of(n) < kHistogramMaxBlocks ? blocks_of(n) : kHistogramMaxBlocks;
    hipLaunchKernelGGL(k_display_histogram, dim3(blocks), dim3(kDisplayBlock), 0, st, d_img, d_pixels, n, d_slots);
}

void launch_display_map(const double* d_img, const int32_t* d_pixels, long long n, const DisplayMap& m, bool rgba, uint8_t* d_out, hipStream_t st)
{
    const bool aligned = reinterpret_cast<uintptr_t>(d_img) % 16 == 0 && reinterpret_cast<uintptr_t>(d_out) % (rgba ? 16 : 4) == 0;
    const bool whole = !d_pixels && aligned;
    if (n <= 0) return;
    if (whole) {
        const unsigned blocks = blocks_of((n >> 2) + 1);       // the full lanes and the one that takes the tail
        if (rgba) hipLaunchKernelGGL(k_display_map<true>, dim3(blocks), dim3(kDisplayBlock), 0, st, d_img, n, m, d_out);
        else hipLaunchKernelGGL(k_display_map<false>, dim3(blocks), dim3(kDisplayBlock), 0, st, d_img, n, m, d_out);
    } else {
        if (rgba) hipLaunchKernelGGL(k_display_map_list<true>, dim3(blocks_of(n)), dim3(kDisplayBlock), 0, st, d_img, d_pixels, n, m, d_out);
        else hipLaunchKernelGGL(k_display_map_list<false>, dim3(blocks_of(n)), dim3(kDisplayBlock), 0, st, d_img, d_pixels, n, m, d_out);
    }
}

}  // namespace mcpt
