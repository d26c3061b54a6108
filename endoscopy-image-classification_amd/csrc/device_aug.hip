// Device input path: the reference's training transforms -- TransformFixMatch (code/dataset.py:24-56,
// code/randaugment.py:147-222), TransformCoMatch (:58-110) and the labeled train transform (:185-196) -- on the
// GPU, from decoded RGB frames of ragged sizes to the planar uint8 [n, 3, S, S] batches es_patch_im2col_u8
// consumes -- byte for byte what esh_transform_batch writes for the same (seed, index).  The host resolves every
// random draw and every double-precision parameter into one plan entry per image (csrc/host_aug.cpp:
// esh_*_device_plan; include/endossl_aug_plan.h); the kernels here are line-by-line ports of host_aug.cpp's
// pixel loops, in integer and fp32 arithmetic.  The doubles are the ones that depend on the pixels: autocontrast's
// LUT, Contrast's mean gray, and ColorJitter's hue (Pillow's HSV round trip, per pixel, with the host's float and
// double types at every step; fmod / floor / round / the divisions are the IEEE ones, no fast-math anywhere).
//
// This file is compiled with -ffp-contract=off, as the host library is: the blends d + alpha * (p - d), the
// 3x3 SMOOTH sum, i * scale + offset and the HSV expressions must round after the multiply AND after the add.
//
//   resize_h_kernel        Image.resize's horizontal pass (resize_h): frame [h][w] -> tmp [h][R]
//   resize_v_crop_kernel   the vertical pass (resize_v), planar out: the CenterCrop window only (and, for
//                          CoMatch, the weak view beside it with its flip), or the whole R x R image (labeled)
//   strong_kernel          one workgroup per image: flip -> reflect crop -> op 0 -> op 1 -> Cutout -> planar
//                          store; the image ping-pongs between two global HWC buffers, barriers between phases
//   jitter_kernel          one workgroup per image: flip folded into the load (a pixel permutation commutes with
//                          every op of the chain) -> up to four ColorJitter ops in the plan's order -> grayscale,
//                          in place in the planar output
//   labeled_kernel         one workgroup per image: the S x S window of the flipped, rotated R x R image in
//                          one gather, then the jitter chain
#include "common.h"

#include <algorithm>
#include <cstddef>

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
  const char* entries;   // any entry type: each begins with EsAugHead's fields
  size_t entry_stride;
  const int32_t* coeffs;
  size_t coeff_count;
  int S, R, max_h;
  u8* tmp;            // [n][max_h][R][3]
  size_t tmp_stride;  // max_h * R * 3
  u8* out;            // [n][3][S][S], or [n][3][R][R] with `full`
  int full;           // the vertical pass keeps the whole R x R image instead of the CenterCrop window
  u8* flipped;        // optional second output [n][3][S][S]: `out` under the entry's flip draw at flip_off
  int flip_off;
};

__device__ __forceinline__ EsAugHead head_of(const ResizeArgs& a, int im) {
  return *(const EsAugHead*)(a.entries + (size_t)im * a.entry_stride);
}

// An entry the kernels can run without leaving the arena, the tables or the temporary; anything else is
// skipped (its outputs are left as they were).
__device__ bool entry_ok(const EsAugHead& e, const ResizeArgs& a) {
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
  const EsAugHead e = head_of(a, im);
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

// resize_v at the S x S CenterCrop window (center_crop's offset is in the entry) or over the whole R x R image,
// or the plain copy when the height already equals R; source = the horizontal pass's output, or the frame itself
// when w == R
__global__ __launch_bounds__(256) void resize_v_crop_kernel(ResizeArgs a) {
  const int im = blockIdx.y;
  const EsAugHead e = head_of(a, im);
  if (!entry_ok(e, a)) return;
  const int R = a.R, S = a.full ? R : a.S, npx = S * S, off = a.full ? 0 : e.crop;
  const u8* src = e.coef_h >= 0 ? a.tmp + (size_t)im * a.tmp_stride : a.frames + e.frame_off;
  const size_t rowb = (size_t)R * 3;
  u8* out = a.out + (size_t)im * 3 * npx;
  u8* fl = a.flipped ? a.flipped + (size_t)im * 3 * npx : nullptr;
  const int flip = fl ? *(const int32_t*)(a.entries + (size_t)im * a.entry_stride + a.flip_off) : 0;
  const int32_t* bounds = e.coef_v >= 0 ? a.coeffs + e.coef_v : nullptr;
  const int32_t* kk = bounds ? bounds + 2 * R : nullptr;
  for (int id = blockIdx.x * blockDim.x + threadIdx.x; id < npx; id += gridDim.x * blockDim.x) {
    const int y = id / S, x = id - y * S;
    const int yy = off + y, xb = (off + x) * 3;
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
    if (fl) {
      const int fid = flip ? y * S + (S - 1 - x) : id;
      fl[fid] = v0;
      fl[npx + fid] = v1;
      fl[2 * npx + fid] = v2;
    }
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

__device__ __forceinline__ int luma(int r, int g, int b) { return (r * 19595 + g * 38470 + b * 7471 + 0x8000) >> 16; }

// Image.blend: deg + alpha * (img - deg) in fp32, truncated; clipped when alpha is outside [0, 1]
__device__ __forceinline__ u8 blend1(int p, int d, float alpha) {
  const float t = (float)d + alpha * (float)(p - d);
  if (alpha >= 0.0f && alpha <= 1.0f) return (u8)(int)t;
  return t <= 0.0f ? 0 : (t >= 255.0f ? 255 : (u8)(int)t);
}

constexpr int STRONG_THREADS = 1024;

// The ImageEnhance blends, shared by the strong chain (HWC: pixel stride ps = 3, channel stride cs = 1) and the
// jitter chain (planar: ps = 1, cs = S * S).  Every thread of the workgroup calls them.
__device__ void blend_brightness(u8* im, int npx, int ps, int cs, float alpha) {  // against black
  for (int i = threadIdx.x; i < npx; i += blockDim.x)
    for (int c = 0; c < 3; ++c) {
      u8* q = im + i * ps + c * cs;
      *q = blend1(*q, 0, alpha);
    }
}

__device__ void blend_color(u8* im, int npx, int ps, int cs, float alpha) {  // against the gray image
  for (int i = threadIdx.x; i < npx; i += blockDim.x) {
    u8* q = im + i * ps;
    const int p0 = q[0], p1 = q[cs], p2 = q[2 * cs], l = luma(p0, p1, p2);
    q[0] = blend1(p0, l, alpha);
    q[cs] = blend1(p1, l, alpha);
    q[2 * cs] = blend1(p2, l, alpha);
  }
}

// against the mean gray of the image as it stands, (int)(sum of i * hist[i] / n + 0.5); hist: 256 ints of LDS
__device__ void blend_contrast(u8* im, int npx, int ps, int cs, float alpha, int* hist, int* mean) {
  const int tid = threadIdx.x, nt = blockDim.x;
  for (int i = tid; i < 256; i += nt) hist[i] = 0;
  __syncthreads();
  for (int i = tid; i < npx; i += nt) {
    const u8* q = im + i * ps;
    atomicAdd(&hist[luma(q[0], q[cs], q[2 * cs])], 1);
  }
  __syncthreads();
  if (tid == 0) {
    double sum = 0.0;
    for (int i = 0; i < 256; ++i) sum += (double)i * (double)hist[i];
    *mean = (int)(sum / (double)npx + 0.5);
  }
  __syncthreads();
  const int dv = *mean;
  for (int i = tid; i < npx; i += nt)
    for (int c = 0; c < 3; ++c) {
      u8* q = im + i * ps + c * cs;
      *q = blend1(*q, dv, alpha);
    }
}

// plans: image im's EsAugStrong at plans + im * stride (EsAugEntry's tail, or EsAugCoEntry's s0)
__global__ __launch_bounds__(STRONG_THREADS) void strong_kernel(const u8* __restrict__ weak,
                                                                const char* __restrict__ plans, size_t stride, int S,
                                                                u8* __restrict__ strong, u8* ws) {
  __shared__ EsAugStrong e;
  __shared__ int hist[3][256];
  __shared__ int lut[3][256];
  __shared__ int lohi[3][2];
  __shared__ int mean;
  const int tid = threadIdx.x, nt = blockDim.x, im = blockIdx.x;
  const int npx = S * S, nb = npx * 3;
  for (int i = tid; i < (int)(sizeof(EsAugStrong) / 4); i += nt)
    ((int32_t*)&e)[i] = ((const int32_t*)(plans + (size_t)im * stride))[i];
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
      case 1: blend_brightness(cur, npx, 3, 1, alpha); break;
      case 2: blend_color(cur, npx, 3, 1, alpha); break;
      case 3: blend_contrast(cur, npx, 3, 1, alpha, hist[0], &mean); break;
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

// ---- the jitter chain -----------------------------------------------------------------------------------
// ColorJitter's hue: host_aug.cpp's rgb2hsv_px -> h += shift (mod 256) -> hsv2rgb_px, expression by expression
// with the same float and double types (Pillow's Convert.c, "following colorsys.py").
__device__ __forceinline__ u8 clip_i(int v) { return (u8)(v < 0 ? 0 : (v > 255 ? 255 : v)); }

__device__ __forceinline__ void hue_px(u8 r, u8 g, u8 b, int shift, u8* out) {
  const u8 maxc = max(r, max(g, b)), minc = min(r, min(g, b));
  u8 uh = 0, us = 0;
  if (minc != maxc) {
    const float cr = (float)(maxc - minc);
    const float sat = cr / (float)maxc;
    const float rc = (float)(maxc - r) / cr, gc = (float)(maxc - g) / cr, bc = (float)(maxc - b) / cr;
    float h;
    if (r == maxc) h = bc - gc;
    else if (g == maxc) h = (float)(2.0 + rc - bc);
    else h = (float)(4.0 + gc - rc);
    h = (float)fmod(h / 6.0 + 1.0, 1.0);
    const int ih = (int)(h * 255.0), is = (int)(sat * 255.0);
    uh = (u8)(ih < 0 ? 0 : (ih > 255 ? 255 : ih));
    us = (u8)(is < 0 ? 0 : (is > 255 ? 255 : is));
  }
  const u8 h = (u8)((uh + shift) & 255), s = us, v = maxc;
  if (s == 0) {
    out[0] = out[1] = out[2] = v;
    return;
  }
  const int i = (int)floor((float)h * 6.0 / 255.0);
  const float f = (float)((float)h * 6.0 / 255.0 - (float)i);
  const float fs = (float)((float)s / 255.0);
  const u8 up = clip_i((int)round((float)v * (1.0 - fs)));
  const u8 uq = clip_i((int)round((float)v * (1.0 - fs * f)));
  const u8 ut = clip_i((int)round((float)v * (1.0 - fs * (1.0 - f))));
  switch (i % 6) {
    case 0: out[0] = v; out[1] = ut; out[2] = up; break;
    case 1: out[0] = uq; out[1] = v; out[2] = up; break;
    case 2: out[0] = up; out[1] = v; out[2] = ut; break;
    case 3: out[0] = up; out[1] = uq; out[2] = v; break;
    case 4: out[0] = ut; out[1] = up; out[2] = v; break;
    default: out[0] = v; out[1] = up; out[2] = uq; break;
  }
}

// The plan's ops in its order, then RandomGrayscale, in place on the planar image im [3][npx]; every thread
// of the workgroup calls it.  hist: 256 ints of LDS.
__device__ void jitter_chain(u8* im, int npx, const EsAugJitter& j, int* hist, int* mean) {
  const int tid = threadIdx.x, nt = blockDim.x;
  for (int k = 0; k < 4; ++k) {
    switch (j.kind[k]) {
      case ES_JIT_BRIGHTNESS: blend_brightness(im, npx, 1, npx, j.factor[0]); break;
      case ES_JIT_CONTRAST: blend_contrast(im, npx, 1, npx, j.factor[1], hist, mean); break;
      case ES_JIT_SATURATION: blend_color(im, npx, 1, npx, j.factor[2]); break;
      case ES_JIT_HUE: {
        const int shift = j.hue;
        for (int i = tid; i < npx; i += nt) {
          u8 o[3];
          hue_px(im[i], im[npx + i], im[2 * npx + i], shift, o);
          im[i] = o[0];
          im[npx + i] = o[1];
          im[2 * npx + i] = o[2];
        }
        break;
      }
      default: break;  // ES_JIT_NONE
    }
    __syncthreads();
  }
  if (j.gray)  // rgb_to_grayscale(img, 3): luma replicated
    for (int i = tid; i < npx; i += nt) {
      const u8 l = (u8)luma(im[i], im[npx + i], im[2 * npx + i]);
      im[i] = im[npx + i] = im[2 * npx + i] = l;
    }
}

// plans: image im's EsAugJitter at plans + im * stride (an EsAugJitter array, or EsAugCoEntry's jit)
__global__ __launch_bounds__(STRONG_THREADS) void jitter_kernel(const u8* __restrict__ base,
                                                                const char* __restrict__ plans, size_t stride, int S,
                                                                u8* __restrict__ out) {
  __shared__ EsAugJitter j;
  __shared__ int hist[256];
  __shared__ int mean;
  const int tid = threadIdx.x, nt = blockDim.x, im = blockIdx.x;
  const int npx = S * S;
  for (int i = tid; i < (int)(sizeof(EsAugJitter) / 4); i += nt)
    ((int32_t*)&j)[i] = ((const int32_t*)(plans + (size_t)im * stride))[i];
  __syncthreads();
  const u8* src = base + (size_t)im * 3 * npx;
  u8* dst = out + (size_t)im * 3 * npx;
  const int flip = j.flip;
  for (int i = tid; i < npx; i += nt) {
    const int y = i / S, x = i - y * S;
    const int si = flip ? y * S + (S - 1 - x) : i;
    dst[i] = src[si];
    dst[npx + i] = src[npx + si];
    dst[2 * npx + i] = src[2 * npx + si];
  }
  __syncthreads();
  jitter_chain(dst, npx, j, hist, &mean);
}

// full: the resized R x R images, planar.  Output (x, y) is pixel (x + crop, y + crop) of the rotated image:
// Pillow's 16.16 walk in closed form (black outside R x R), over the image flipped as the plan says.
__global__ __launch_bounds__(STRONG_THREADS) void labeled_kernel(const u8* __restrict__ full,
                                                                 const EsAugLabEntry* __restrict__ entries, int S,
                                                                 int R, u8* __restrict__ out) {
  __shared__ EsAugLabEntry e;
  __shared__ int hist[256];
  __shared__ int mean;
  const int tid = threadIdx.x, nt = blockDim.x, im = blockIdx.x;
  const int npx = S * S, rpx = R * R;
  for (int i = tid; i < (int)(sizeof(EsAugLabEntry) / 4); i += nt) ((int32_t*)&e)[i] = ((const int32_t*)(entries + im))[i];
  __syncthreads();
  const int crop = e.head.crop;
  if (crop < 0 || crop + S > R) return;  // the whole workgroup: such an entry is skipped, as the resize skips it
  const u8* src = full + (size_t)im * 3 * rpx;
  u8* dst = out + (size_t)im * 3 * npx;
  const int rot = e.rot, hflip = e.hflip, vflip = e.vflip;
  const unsigned a0 = e.a[0], a1 = e.a[1], a2 = e.a[2], a3 = e.a[3], a4 = e.a[4], a5 = e.a[5];
  for (int i = tid; i < npx; i += nt) {
    const int y = i / S, x = i - y * S;
    int xi = x + crop, yi = y + crop;
    if (rot) {
      const int xx = (int)(a2 + (unsigned)yi * a1 + (unsigned)xi * a0);
      const int yy = (int)(a5 + (unsigned)yi * a4 + (unsigned)xi * a3);
      xi = xx >> 16;  // arithmetic shift = floor
      yi = yy >> 16;
    }
    u8 v0 = 0, v1 = 0, v2 = 0;
    if (xi >= 0 && xi < R && yi >= 0 && yi < R) {
      const int si = (vflip ? R - 1 - yi : yi) * R + (hflip ? R - 1 - xi : xi);
      v0 = src[si];
      v1 = src[rpx + si];
      v2 = src[2 * rpx + si];
    }
    dst[i] = v0;
    dst[npx + i] = v1;
    dst[2 * npx + i] = v2;
  }
  __syncthreads();
  jitter_chain(dst, npx, e.jit, hist, &mean);
}

constexpr int MAX_S = 4096;  // keeps every per-image index in int32

size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

bool shape_ok(int n, int S) { return n > 0 && n <= 65535 && S >= 2 && S <= MAX_S && (int)(S * 0.125) < S; }

int resize_side(int S, int is_crop) { return is_crop ? (int)(S * 1.2) : S; }

// The refusals every frames -> batch call shares, all before any launch; *tmp_bytes = the horizontal pass's
// temporary, the first region of the workspace
int resize_check(const uint8_t* frames, size_t frames_bytes, const void* entries, const int32_t* coeffs,
                 size_t coeff_count, int n, int S, int is_crop, int max_h, const void* workspace, size_t* tmp_bytes) {
  if (!shape_ok(n, S) || max_h <= 0) return ES_BAD_SHAPE;
  const int R = resize_side(S, is_crop);
  if (R < S || (size_t)max_h * R * 3 > (size_t)INT32_MAX) return ES_BAD_SHAPE;
  if (!frames || !frames_bytes || !entries || !workspace || ((uintptr_t)entries & 7) || ((uintptr_t)coeffs & 3))
    return ES_BAD_ARG;
  if (!coeffs && coeff_count) return ES_BAD_ARG;
  *tmp_bytes = align256((size_t)n * max_h * R * 3);
  return ES_OK;
}

// both resize passes; a.out / full / flipped / flip_off say what the vertical one writes
void launch_resize(ResizeArgs a, const uint8_t* frames, size_t frames_bytes, const void* entries, size_t entry_stride,
                   const int32_t* coeffs, size_t coeff_count, int n, int S, int is_crop, int max_h, void* workspace,
                   hipStream_t stream) {
  a.frames = frames;
  a.frames_bytes = frames_bytes;
  a.entries = (const char*)entries;
  a.entry_stride = entry_stride;
  a.coeffs = coeffs;
  a.coeff_count = coeff_count;
  a.S = S;
  a.R = resize_side(S, is_crop);
  a.max_h = max_h;
  a.tmp = (u8*)workspace;
  a.tmp_stride = (size_t)max_h * a.R * 3;
  const int bh = (int)std::min<size_t>(((size_t)max_h * a.R + 255) / 256, 2048);
  hipLaunchKernelGGL(resize_h_kernel, dim3(bh, n), 256, 0, stream, a);
  const int side = a.full ? a.R : S;
  const int bv = std::min((side * side + 255) / 256, 2048);
  hipLaunchKernelGGL(resize_v_crop_kernel, dim3(bv, n), 256, 0, stream, a);
}

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
  return align256((size_t)n * max_h * resize_side(S, is_crop) * 3) + es_aug_strong_workspace(n, S);
}

int es_aug_strong_u8(const uint8_t* weak, const void* entries, int n, int S, uint8_t* strong, void* workspace,
                     size_t workspace_bytes, hipStream_t stream) {
  if (!shape_ok(n, S)) return ES_BAD_SHAPE;
  if (!weak || !entries || !strong || !workspace || ((uintptr_t)entries & 7)) return ES_BAD_ARG;
  if (workspace_bytes < es_aug_strong_workspace(n, S)) return ES_BAD_ARG;
  hipLaunchKernelGGL(strong_kernel, n, STRONG_THREADS, 0, stream, weak, (const char*)entries + offsetof(EsAugEntry, flip),
                     sizeof(EsAugEntry), S, strong, (u8*)workspace);
  return hipGetLastError() == hipSuccess ? ES_OK : ES_HIP_ERROR;
}

int es_aug_fixmatch_u8(const uint8_t* frames, size_t frames_bytes, const void* entries, const int32_t* coeffs,
                       size_t coeff_count, int n, int S, int is_crop, int max_h, uint8_t* weak, uint8_t* strong,
                       void* workspace, size_t workspace_bytes, hipStream_t stream) {
  size_t tmp_bytes = 0;
  const int rc = resize_check(frames, frames_bytes, entries, coeffs, coeff_count, n, S, is_crop, max_h, workspace,
                              &tmp_bytes);
  if (rc != ES_OK) return rc;
  if (!weak) return ES_BAD_ARG;
  if (workspace_bytes < tmp_bytes + (strong ? es_aug_strong_workspace(n, S) : 0)) return ES_BAD_ARG;
  ResizeArgs a = {};
  a.out = weak;
  launch_resize(a, frames, frames_bytes, entries, sizeof(EsAugEntry), coeffs, coeff_count, n, S, is_crop, max_h,
                workspace, stream);
  if (strong)
    hipLaunchKernelGGL(strong_kernel, n, STRONG_THREADS, 0, stream, (const u8*)weak,
                       (const char*)entries + offsetof(EsAugEntry, flip), sizeof(EsAugEntry), S, strong,
                       (u8*)workspace + tmp_bytes);
  return hipGetLastError() == hipSuccess ? ES_OK : ES_HIP_ERROR;
}

// ---- TransformCoMatch: four launches ------------------------------------------------------------------------
size_t es_aug_comatch_entry_size(void) { return sizeof(EsAugCoEntry); }

// the horizontal pass's temporary, the unflipped base views, the strong chain's ping-pong images
size_t es_aug_comatch_workspace(int n, int S, int is_crop, int max_w, int max_h) {
  if (!shape_ok(n, S) || max_w <= 0 || max_h <= 0) return 0;
  return align256((size_t)n * max_h * resize_side(S, is_crop) * 3) + align256((size_t)n * 3 * S * S) +
         es_aug_strong_workspace(n, S);
}

int es_aug_comatch_u8(const uint8_t* frames, size_t frames_bytes, const void* entries, const int32_t* coeffs,
                      size_t coeff_count, int n, int S, int is_crop, int max_h, uint8_t* weak, uint8_t* strong0,
                      uint8_t* strong1, void* workspace, size_t workspace_bytes, hipStream_t stream) {
  size_t tmp_bytes = 0;
  const int rc = resize_check(frames, frames_bytes, entries, coeffs, coeff_count, n, S, is_crop, max_h, workspace,
                              &tmp_bytes);
  if (rc != ES_OK) return rc;
  if (!weak || !strong0 || !strong1) return ES_BAD_ARG;
  const size_t base_bytes = align256((size_t)n * 3 * S * S);
  if (workspace_bytes < tmp_bytes + base_bytes + es_aug_strong_workspace(n, S)) return ES_BAD_ARG;
  u8* base = (u8*)workspace + tmp_bytes;
  ResizeArgs a = {};
  a.out = base;
  a.flipped = weak;
  a.flip_off = (int)offsetof(EsAugCoEntry, flip_w);
  launch_resize(a, frames, frames_bytes, entries, sizeof(EsAugCoEntry), coeffs, coeff_count, n, S, is_crop, max_h,
                workspace, stream);
  const char* ent = (const char*)entries;
  hipLaunchKernelGGL(strong_kernel, n, STRONG_THREADS, 0, stream, (const u8*)base, ent + offsetof(EsAugCoEntry, s0),
                     sizeof(EsAugCoEntry), S, strong0, base + base_bytes);
  hipLaunchKernelGGL(jitter_kernel, n, STRONG_THREADS, 0, stream, (const u8*)base, ent + offsetof(EsAugCoEntry, jit),
                     sizeof(EsAugCoEntry), S, strong1);
  return hipGetLastError() == hipSuccess ? ES_OK : ES_HIP_ERROR;
}

// ---- the labeled train transform: three launches ---------------------------------------------------------------
size_t es_aug_labeled_entry_size(void) { return sizeof(EsAugLabEntry); }

// the horizontal pass's temporary, the whole resized R x R images
size_t es_aug_labeled_workspace(int n, int S, int is_crop, int max_w, int max_h) {
  if (!shape_ok(n, S) || max_w <= 0 || max_h <= 0) return 0;
  const int R = resize_side(S, is_crop);
  return align256((size_t)n * max_h * R * 3) + (size_t)n * 3 * R * R;
}

int es_aug_labeled_u8(const uint8_t* frames, size_t frames_bytes, const void* entries, const int32_t* coeffs,
                      size_t coeff_count, int n, int S, int is_crop, int max_h, uint8_t* out, void* workspace,
                      size_t workspace_bytes, hipStream_t stream) {
  size_t tmp_bytes = 0;
  const int rc = resize_check(frames, frames_bytes, entries, coeffs, coeff_count, n, S, is_crop, max_h, workspace,
                              &tmp_bytes);
  if (rc != ES_OK) return rc;
  if (!out) return ES_BAD_ARG;
  const int R = resize_side(S, is_crop);
  if (workspace_bytes < tmp_bytes + (size_t)n * 3 * R * R) return ES_BAD_ARG;
  u8* full = (u8*)workspace + tmp_bytes;
  ResizeArgs a = {};
  a.out = full;
  a.full = 1;
  launch_resize(a, frames, frames_bytes, entries, sizeof(EsAugLabEntry), coeffs, coeff_count, n, S, is_crop, max_h,
                workspace, stream);
  hipLaunchKernelGGL(labeled_kernel, n, STRONG_THREADS, 0, stream, (const u8*)full, (const EsAugLabEntry*)entries, S, R,
                     out);
  return hipGetLastError() == hipSuccess ? ES_OK : ES_HIP_ERROR;
}

// One jitter chain (flip, the ops in order, grayscale) over S x S planar views x under explicit plans (n
// EsAugJitter, 4-byte aligned); out must not be x.
int es_aug_jitter_u8(const uint8_t* x, const void* plans, int n, int S, uint8_t* out, hipStream_t stream) {
  if (!shape_ok(n, S)) return ES_BAD_SHAPE;
  if (!x || !plans || !out || x == out || ((uintptr_t)plans & 3)) return ES_BAD_ARG;
  hipLaunchKernelGGL(jitter_kernel, n, STRONG_THREADS, 0, stream, x, (const char*)plans, sizeof(EsAugJitter), S, out);
  return hipGetLastError() == hipSuccess ? ES_OK : ES_HIP_ERROR;
}

}  // extern "C"
