// Device input path: the reference's TransformFixMatch (code/dataset.py:24-56, code/randaugment.py:147-222)
// on the GPU, from decoded RGB frames of ragged sizes to the planar uint8 (weak, strong) [n, 3, S, S] batches
// es_patch_im2col_u8 consumes -- byte for byte what esh_transform_batch(kind 0) writes for the same
// (seed, index).  The host resolves every random draw and every double-precision parameter into one
// EsAugEntry per image (csrc/host_aug.cpp: esh_fixmatch_device_plan; include/endossl_aug_plan.h); the kernels
// here are line-by-line ports of host_aug.cpp's pixel loops, in integer and fp32 arithmetic.  The only doubles
// are the two histogram-dependent ones the plan cannot hold: autocontrast's LUT and Contrast's mean gray.
//
// This file is compiled with -ffp-contract=off, as the host library is: the blends d + alpha * (p - d), the
// 3x3 SMOOTH sum and i * scale + offset must round after the multiply AND after the add.
//
//   resize_h_kernel        Image.resize's horizontal pass (resize_h): frame [h][w] -> tmp [h][R]
//   resize_v_crop_kernel   the vertical pass (resize_v) at the CenterCrop window only, planar weak view out
//   strong_kernel          one workgroup per image: flip -> reflect crop -> op 0 -> op 1 -> Cutout -> planar
//                          store; the image ping-pongs between two global HWC buffers, barriers between phases
#include "common.h"

#include <algorithm>

#include "../../include/endossl_aug_plan.h"

namespace {

typedef uint8_t u8;
constexpr int PREC = 32 - 8 - 2;  // Pillow's coefficient precision

__device__ __forceinline__ u8 clip8(int v) {
  v >>= PREC;
  return v < 0 ? 0 : (v > 255 ? 255 : (u8)v);
}

struct ResizeArgs {
  const u8* frames;
  size_t frames_bytes;
  const EsAugEntry* entries;
  const int32_t* coeffs;
  size_t coeff_count;
  int S, R, max_h;
  u8* tmp;            // [n][max_h][R][3]
  size_t tmp_stride;  // max_h * R * 3
  u8* weak;           // [n][3][S][S]
};

// An entry the kernels can run without leaving the arena, the tables or the temporary; anything else is
// skipped (its outputs are left as they were).
__device__ bool entry_ok(const EsAugEntry& e, const ResizeArgs& a) {
  if (e.w <= 0 || e.h <= 0 || e.h > a.max_h || e.frame_off < 0) return false;
  if ((uint64_t)e.frame_off + (uint64_t)e.w * (uint64_t)e.h * 3u > (uint64_t)a.frames_bytes) return false;
  if ((e.coef_h < 0) != (e.w == a.R) || (e.coef_v < 0) != (e.h == a.R)) return false;
  if (e.coef_h >= 0 && (e.ksize_h <= 0 || (uint64_t)e.coef_h + (uint64_t)a.R * (2u + e.ksize_h) > a.coeff_count))
    return false;
  if (e.coef_v >= 0 && (e.ksize_v <= 0 || (uint64_t)e.coef_v + (uint64_t)a.R * (2u + e.ksize_v) > a.coeff_count))
    return false;
  return e.crop >= 0 && e.crop + a.S <= a.R;
}

// resize_h: every row of the frame, R output columns
__global__ __launch_bounds__(256) void resize_h_kernel(ResizeArgs a) {
  const int im = blockIdx.y;
  const EsAugEntry e = a.entries[im];
  if (e.coef_h < 0 || !entry_ok(e, a)) return;
  const int R = a.R;
  const u8* src = a.frames + e.frame_off;
  u8* dst = a.tmp + (size_t)im * a.tmp_stride;
  const int32_t* bounds = a.coeffs + e.coef_h;
  const int32_t* kk = bounds + 2 * R;
  const int total = e.h * R;
  for (int id = blockIdx.x * blockDim.x + threadIdx.x; id < total; id += gridDim.x * blockDim.x) {
    const int y = id / R, xx = id - y * R;
    int xmin = bounds[xx * 2], xmax = bounds[xx * 2 + 1];
    xmin = max(xmin, 0);
    xmax = min(min(xmax, e.ksize_h), e.w - xmin);  // a table the host wrote never trips these
    const int32_t* k = kk + (size_t)xx * e.ksize_h;
    const u8* s = src + (size_t)y * e.w * 3;
    int s0 = 1 << (PREC - 1), s1 = s0, s2 = s0;
    for (int x = 0; x < xmax; ++x) {
      const u8* q = s + (x + xmin) * 3;
      s0 += q[0] * k[x];
      s1 += q[1] * k[x];
      s2 += q[2] * k[x];
    }
    u8* d = dst + (size_t)id * 3;
    d[0] = clip8(s0);
    d[1] = clip8(s1);
    d[2] = clip8(s2);
  }
}

// resize_v at the S x S CenterCrop window (center_crop's offset is in the entry), or the plain copy when the
// height already equals R; source = the horizontal pass's output, or the frame itself when w == R
__global__ __launch_bounds__(256) void resize_v_crop_kernel(ResizeArgs a) {
  const int im = blockIdx.y;
  const EsAugEntry e = a.entries[im];
  if (!entry_ok(e, a)) return;
  const int R = a.R, S = a.S, npx = S * S;
  const u8* src = e.coef_h >= 0 ? a.tmp + (size_t)im * a.tmp_stride : a.frames + e.frame_off;
  const size_t rowb = (size_t)R * 3;
  u8* out = a.weak + (size_t)im * 3 * npx;
  const int32_t* bounds = e.coef_v >= 0 ? a.coeffs + e.coef_v : nullptr;
  const int32_t* kk = bounds ? bounds + 2 * R : nullptr;
  for (int id = blockIdx.x * blockDim.x + threadIdx.x; id < npx; id += gridDim.x * blockDim.x) {
    const int y = id / S, x = id - y * S;
    const int yy = e.crop + y, xb = (e.crop + x) * 3;
    u8 v0, v1, v2;
    if (!bounds) {
      const u8* q = src + yy * rowb + xb;
      v0 = q[0];
      v1 = q[1];
      v2 = q[2];
    } else {
      int ymin = bounds[yy * 2], ymax = bounds[yy * 2 + 1];
      ymin = max(ymin, 0);
      ymax = min(min(ymax, e.ksize_v), e.h - ymin);
      const int32_t* k = kk + (size_t)yy * e.ksize_v;
      int s0 = 1 << (PREC - 1), s1 = s0, s2 = s0;
      for (int t = 0; t < ymax; ++t) {
        const u8* q = src + (size_t)(t + ymin) * rowb + xb;
        s0 += q[0] * k[t];
        s1 += q[1] * k[t];
        s2 += q[2] * k[t];
      }
      v0 = clip8(s0);
      v1 = clip8(s1);
      v2 = clip8(s2);
    }
    out[id] = v0;
    out[npx + id] = v1;
    out[2 * npx + id] = v2;
  }
}

// ---- the strong chain ---------------------------------------------------------------------------------
__device__ __forceinline__ int reflect_idx(int i, int n) {  // numpy pad mode 'reflect'
  if (n == 1) return 0;
  const int period = 2 * (n - 1);
  i %= period;
  if (i < 0) i += period;
  return i < n ? i : period - i;
}

__device__ __forceinline__ int luma(const u8* q) { return (q[0] * 19595 + q[1] * 38470 + q[2] * 7471 + 0x8000) >> 16; }

// Image.blend: deg + alpha * (img - deg) in fp32, truncated; clipped when alpha is outside [0, 1]
__device__ __forceinline__ u8 blend1(int p, int d, float alpha) {
  const float t = (float)d + alpha * (float)(p - d);
  if (alpha >= 0.0f && alpha <= 1.0f) return (u8)(int)t;
  return t <= 0.0f ? 0 : (t >= 255.0f ? 255 : (u8)(int)t);
}

constexpr int STRONG_THREADS = 1024;

__global__ __launch_bounds__(STRONG_THREADS) void strong_kernel(const u8* __restrict__ weak,
                                                                const EsAugEntry* __restrict__ entries, int S,
                                                                u8* __restrict__ strong, u8* ws) {
  __shared__ EsAugEntry e;
  __shared__ int hist[3][256];
  __shared__ int lut[3][256];
  __shared__ int lohi[3][2];
  __shared__ int mean;
  const int tid = threadIdx.x, nt = blockDim.x, im = blockIdx.x;
  const int npx = S * S, nb = npx * 3;
  for (int i = tid; i < (int)(sizeof(EsAugEntry) / 4); i += nt) ((int32_t*)&e)[i] = ((const int32_t*)(entries + im))[i];
  __syncthreads();
  const u8* wk = weak + (size_t)im * nb;
  u8* cur = ws + (size_t)im * 2 * nb;  // HWC
  u8* oth = cur + nb;

  // RandomHorizontalFlip, then RandomCrop(S, padding=pad, reflect) at (top, left)
  {
    const int pad = (int)(S * 0.125f);  // S / 8, exact in fp32 for any S the launcher admits
    const int flip = e.flip, top = e.top, left = e.left;
    for (int i = tid; i < npx; i += nt) {
      const int y = i / S, x = i - y * S;
      const int sy = reflect_idx(top + y - pad, S);
      int sx = reflect_idx(left + x - pad, S);
      if (flip) sx = S - 1 - sx;
      const int si = sy * S + sx;
      cur[i * 3] = wk[si];
      cur[i * 3 + 1] = wk[npx + si];
      cur[i * 3 + 2] = wk[2 * npx + si];
    }
  }
  __syncthreads();

  for (int slot = 0; slot < 2; ++slot) {
    const int kind = e.ops[slot].kind;
    const float alpha = e.ops[slot].alpha;
    switch (kind) {
      case 0:    // AutoContrast
      case 4: {  // Equalize: per-channel histograms of the current image, then a LUT per channel
        for (int i = tid; i < 768; i += nt) (&hist[0][0])[i] = 0;
        __syncthreads();
        for (int i = tid; i < nb; i += nt) atomicAdd(&hist[i % 3][cur[i]], 1);
        __syncthreads();
        if (kind == 0) {
          if (tid < 3) {
            int lo = 0, hi = 255;
            while (lo < 255 && !hist[tid][lo]) ++lo;
            while (hi > 0 && !hist[tid][hi]) --hi;
            lohi[tid][0] = lo;
            lohi[tid][1] = hi;
          }
          __syncthreads();
          for (int j = tid; j < 768; j += nt) {
            const int c = j >> 8, i = j & 255, lo = lohi[c][0], hi = lohi[c][1];
            int v = i;
            if (hi > lo) {
              const double scale = 255.0 / (hi - lo), offset = -lo * scale;
              v = (int)(i * scale + offset);
              v = v < 0 ? 0 : (v > 255 ? 255 : v);
            }
            lut[c][i] = v;
          }
        } else if (tid < 3) {
          const int c = tid;
          int total = 0, last = 0, nz = 0;
          for (int i = 0; i < 256; ++i)
            if (hist[c][i]) {
              total += hist[c][i];
              last = hist[c][i];
              ++nz;
            }
          const int step = nz <= 1 ? 0 : (total - last) / 255;
          if (!step) {
            for (int i = 0; i < 256; ++i) lut[c][i] = i;
          } else {
            int n = step / 2;
            for (int i = 0; i < 256; ++i) {
              const int v = n / step;
              lut[c][i] = v > 255 ? 255 : v;
              n += hist[c][i];
            }
          }
        }
        __syncthreads();
        for (int i = tid; i < nb; i += nt) cur[i] = (u8)lut[i % 3][cur[i]];
        break;
      }
      case 1:  // Brightness: blend against black
        for (int i = tid; i < nb; i += nt) cur[i] = blend1(cur[i], 0, alpha);
        break;
      case 2:  // Color: blend against the gray image
        for (int i = tid; i < npx; i += nt) {
          u8* q = cur + i * 3;
          const int l = luma(q);
          const u8 r0 = blend1(q[0], l, alpha), r1 = blend1(q[1], l, alpha), r2 = blend1(q[2], l, alpha);
          q[0] = r0;
          q[1] = r1;
          q[2] = r2;
        }
        break;
      case 3: {  // Contrast: blend against the mean gray, (int)(sum of i * hist[i] / n + 0.5)
        for (int i = tid; i < 256; i += nt) hist[0][i] = 0;
        __syncthreads();
        for (int i = tid; i < npx; i += nt) atomicAdd(&hist[0][luma(cur + i * 3)], 1);
        __syncthreads();
        if (tid == 0) {
          double sum = 0.0;
          for (int i = 0; i < 256; ++i) sum += (double)i * (double)hist[0][i];
          mean = (int)(sum / (double)npx + 0.5);
        }
        __syncthreads();
        const int dv = mean;
        for (int i = tid; i < nb; i += nt) cur[i] = blend1(cur[i], dv, alpha);
        break;
      }
      case 6: {  // Posterize
        const int mask = e.ops[slot].mask;
        for (int i = tid; i < nb; i += nt) cur[i] = (u8)(cur[i] & mask & 255);
        break;
      }
      case 11: {  // Solarize
        const int th = e.ops[slot].thresh;
        for (int i = tid; i < nb; i += nt) {
          const int p = cur[i];
          cur[i] = (u8)(p < th ? p : 255 - p);
        }
        break;
      }
      case 8: {  // Sharpness: blend against ImageFilter.SMOOTH (borders copied)
        constexpr float k1 = 1.0f / 13.0f, k5 = 5.0f / 13.0f;
        const int rb = S * 3;
        for (int i = tid; i < npx; i += nt) {
          const int y = i / S, x = i - y * S;
          const bool inner = y >= 1 && y < S - 1 && x >= 1 && x < S - 1;
          for (int c = 0; c < 3; ++c) {
            const int j = i * 3 + c;
            const int p = cur[j];
            int d = p;
            if (inner) {
              const u8* r1 = cur + j;
              const u8* r0 = r1 - rb;
              const u8* r2 = r1 + rb;
              float ss = 0.0f;
              ss += (float)r2[-3] * k1 + (float)r2[0] * k1 + (float)r2[3] * k1;
              ss += (float)r1[-3] * k1 + (float)r1[0] * k5 + (float)r1[3] * k1;
              ss += (float)r0[-3] * k1 + (float)r0[0] * k1 + (float)r0[3] * k1;
              d = ss <= 0.0f ? 0 : (ss >= 255.0f ? 255 : (u8)(int)(ss + 0.5f));
            }
            oth[j] = blend1(p, d, alpha);
          }
        }
        { u8* t = cur; cur = oth; oth = t; }
        break;
      }
      case 7: case 9: case 10: {  // Rotate / ShearX / ShearY: the 16.16 walk in closed form, black fill
        const unsigned a0 = e.ops[slot].a[0], a1 = e.ops[slot].a[1], a2 = e.ops[slot].a[2];
        const unsigned a3 = e.ops[slot].a[3], a4 = e.ops[slot].a[4], a5 = e.ops[slot].a[5];
        for (int i = tid; i < npx; i += nt) {
          const int y = i / S, x = i - y * S;
          const int xx = (int)(a2 + (unsigned)y * a1 + (unsigned)x * a0);
          const int yy = (int)(a5 + (unsigned)y * a4 + (unsigned)x * a3);
          const int xi = xx >> 16, yi = yy >> 16;  // arithmetic shift = floor
          u8 v0 = 0, v1 = 0, v2 = 0;
          if (xi >= 0 && xi < S && yi >= 0 && yi < S) {
            const u8* q = cur + (yi * S + xi) * 3;
            v0 = q[0];
            v1 = q[1];
            v2 = q[2];
          }
          oth[i * 3] = v0;
          oth[i * 3 + 1] = v1;
          oth[i * 3 + 2] = v2;
        }
        { u8* t = cur; cur = oth; oth = t; }
        break;
      }
      case ES_AUG_SHIFT: {  // TranslateX / TranslateY
        const long long dx = e.ops[slot].shift_x, dy = e.ops[slot].shift_y;
        for (int i = tid; i < npx; i += nt) {
          const int y = i / S, x = i - y * S;
          const long long xi = x + dx, yi = y + dy;
          u8 v0 = 0, v1 = 0, v2 = 0;
          if (xi >= 0 && xi < S && yi >= 0 && yi < S) {
            const u8* q = cur + ((int)yi * S + (int)xi) * 3;
            v0 = q[0];
            v1 = q[1];
            v2 = q[2];
          }
          oth[i * 3] = v0;
          oth[i * 3 + 1] = v1;
          oth[i * 3 + 2] = v2;
        }
        { u8* t = cur; cur = oth; oth = t; }
        break;
      }
      default: break;  // ES_AUG_NONE
    }
    __syncthreads();
  }

  // CutoutAbs: ImageDraw.rectangle, inclusive corners clipped to the image, gray 127; then HWC -> planar
  const int x0 = max(e.rect[0], 0), y0 = max(e.rect[1], 0);
  const int x1 = min(e.rect[2], S - 1), y1 = min(e.rect[3], S - 1);
  u8* out = strong + (size_t)im * nb;
  for (int i = tid; i < npx; i += nt) {
    const int y = i / S, x = i - y * S;
    const bool cut = y >= y0 && y <= y1 && x >= x0 && x <= x1;
    out[i] = cut ? (u8)127 : cur[i * 3];
    out[npx + i] = cut ? (u8)127 : cur[i * 3 + 1];
    out[2 * npx + i] = cut ? (u8)127 : cur[i * 3 + 2];
  }
}

constexpr int MAX_S = 4096;  // keeps every per-image index in int32

size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

bool shape_ok(int n, int S) { return n > 0 && n <= 65535 && S >= 2 && S <= MAX_S && (int)(S * 0.125) < S; }

}  // namespace

extern "C" {

size_t es_aug_entry_size(void) { return sizeof(EsAugEntry); }

// the strong chain's two HWC ping-pong images per batch image
size_t es_aug_strong_workspace(int n, int S) {
  if (!shape_ok(n, S)) return 0;
  return (size_t)n * 6 * S * S;
}

size_t es_aug_fixmatch_workspace(int n, int S, int is_crop, int max_w, int max_h) {
  if (!shape_ok(n, S) || max_w <= 0 || max_h <= 0) return 0;
  const int R = is_crop ? (int)(S * 1.2) : S;
  return align256((size_t)n * max_h * R * 3) + es_aug_strong_workspace(n, S);
}

int es_aug_strong_u8(const uint8_t* weak, const void* entries, int n, int S, uint8_t* strong, void* workspace,
                     size_t workspace_bytes, hipStream_t stream) {
  if (!shape_ok(n, S)) return ES_BAD_SHAPE;
  if (!weak || !entries || !strong || !workspace || ((uintptr_t)entries & 7)) return ES_BAD_ARG;
  if (workspace_bytes < es_aug_strong_workspace(n, S)) return ES_BAD_ARG;
  hipLaunchKernelGGL(strong_kernel, n, STRONG_THREADS, 0, stream, weak, (const EsAugEntry*)entries, S, strong,
                     (u8*)workspace);
  return hipGetLastError() == hipSuccess ? ES_OK : ES_HIP_ERROR;
}

int es_aug_fixmatch_u8(const uint8_t* frames, size_t frames_bytes, const void* entries, const int32_t* coeffs,
                       size_t coeff_count, int n, int S, int is_crop, int max_h, uint8_t* weak, uint8_t* strong,
                       void* workspace, size_t workspace_bytes, hipStream_t stream) {
  if (!shape_ok(n, S) || max_h <= 0) return ES_BAD_SHAPE;
  const int R = is_crop ? (int)(S * 1.2) : S;
  if (R < S || (size_t)max_h * R * 3 > (size_t)INT32_MAX) return ES_BAD_SHAPE;
  if (!frames || !frames_bytes || !entries || !weak || !workspace || ((uintptr_t)entries & 7) ||
      ((uintptr_t)coeffs & 3))
    return ES_BAD_ARG;
  if (!coeffs && coeff_count) return ES_BAD_ARG;
  const size_t tmp_stride = (size_t)max_h * R * 3, tmp_bytes = align256((size_t)n * tmp_stride);
  if (workspace_bytes < tmp_bytes + (strong ? es_aug_strong_workspace(n, S) : 0)) return ES_BAD_ARG;
  ResizeArgs a;
  a.frames = frames;
  a.frames_bytes = frames_bytes;
  a.entries = (const EsAugEntry*)entries;
  a.coeffs = coeffs;
  a.coeff_count = coeff_count;
  a.S = S;
  a.R = R;
  a.max_h = max_h;
  a.tmp = (u8*)workspace;
  a.tmp_stride = tmp_stride;
  a.weak = weak;
  const int bh = (int)std::min<size_t>(((size_t)max_h * R + 255) / 256, 2048);
  hipLaunchKernelGGL(resize_h_kernel, dim3(bh, n), 256, 0, stream, a);
  const int bv = std::min((S * S + 255) / 256, 2048);
  hipLaunchKernelGGL(resize_v_crop_kernel, dim3(bv, n), 256, 0, stream, a);
  if (strong)
    hipLaunchKernelGGL(strong_kernel, n, STRONG_THREADS, 0, stream, (const u8*)weak, (const EsAugEntry*)entries, S,
                       strong, (u8*)workspace + tmp_bytes);
  return hipGetLastError() == hipSuccess ? ES_OK : ES_HIP_ERROR;
}

}  // extern "C"
