// BatchNorm row reductions shared by conv.hip and densenet.hip: per-channel sums over the rows of a (strided)
// [rows, C] view, their second pass, the statistics from a conv epilogue's partials, and the pinned per-element
// arithmetic of the backward.  One definition, so that every caller reduces in the same order (bit-identical).
#pragma once
#include "common.h"

namespace {

// ---- per-channel reductions over the rows of a [rows, C] view: row r at (r / HW) * sn + (r % HW) * sp.
// One workgroup per row chunk writes partial[block][c]; chan_final_kernel sums the blocks.
struct RowMap {
  long sn, sp;
  int HW;
};

// VEC consecutive floats (VEC = 4: one 16-byte load)
template <int VEC>
__device__ __forceinline__ void ldv(const float* __restrict__ p, float (&o)[VEC]) {
  if constexpr (VEC == 4 || VEC == 8) {
#pragma unroll
    for (int h = 0; h < VEC / 4; ++h) {
      const f32x4 t = *(const f32x4*)(p + 4 * h);
      o[4 * h] = t[0]; o[4 * h + 1] = t[1]; o[4 * h + 2] = t[2]; o[4 * h + 3] = t[3];
    }
  } else {
#pragma unroll
    for (int j = 0; j < VEC; ++j) o[j] = p[j];
  }
}
template <int VEC>
__device__ __forceinline__ void stv(float* __restrict__ p, const float (&v)[VEC]) {
  if constexpr (VEC == 4 || VEC == 8) {
#pragma unroll
    for (int h = 0; h < VEC / 4; ++h) *(f32x4*)(p + 4 * h) = f32x4{v[4 * h], v[4 * h + 1], v[4 * h + 2], v[4 * h + 3]};
  } else {
#pragma unroll
    for (int j = 0; j < VEC; ++j) p[j] = v[j];
  }
}
// bf16 maps: VEC consecutive elements widened to fp32 (VEC = 4: one 8-byte load) / rounded once on store
template <int VEC>
__device__ __forceinline__ void ldv(const bf16* __restrict__ p, float (&o)[VEC]) {
  if constexpr (VEC == 4) {
    const bf16x4 t = *(const bf16x4*)p;
    o[0] = (float)t[0]; o[1] = (float)t[1]; o[2] = (float)t[2]; o[3] = (float)t[3];
  } else if constexpr (VEC == 8) {
    const bf16x8 t = *(const bf16x8*)p;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = (float)t[j];
  } else {
#pragma unroll
    for (int j = 0; j < VEC; ++j) o[j] = (float)p[j];
  }
}
template <int VEC>
__device__ __forceinline__ void stv(bf16* __restrict__ p, const float (&v)[VEC]) {
  if constexpr (VEC == 4) {
    *(bf16x4*)p = bf16x4{(bf16)v[0], (bf16)v[1], (bf16)v[2], (bf16)v[3]};
  } else if constexpr (VEC == 8) {
    bf16x8 t;
#pragma unroll
    for (int j = 0; j < 8; ++j) t[j] = (bf16)v[j];
    *(bf16x8*)p = t;
  } else {
#pragma unroll
    for (int j = 0; j < VEC; ++j) p[j] = (bf16)v[j];
  }
}

// The BatchNorm affine map of the forward (bn_affine, common.h): one function for bn_apply_kernel, for the
// backward kernels that rebuild the ReLU mask from x and for the bf16 convs' BatchNorm-applying gathers.
// the forward's y > 0 for a ReLU BatchNorm without residual: relu(affine) rounded to the map type T
template <typename T>
__device__ __forceinline__ bool bn_relu_live(float x, float mu, float rs, float ga, float be) {
  return (float)(T)fmaxf(bn_affine(x, mu, rs, ga, be), 0.f) > 0.f;
}
// MODE 0: sum v;  MODE 1: sum (v - mean[c])^2;  MODE 2: sum g, sum g * xhat  (g = dy * [y > 0 if relu],
// xhat = (x - mean) * rstd), written as partial[block][c] and partial[block][C + c].
// A thread owns VEC channels and walks every rp-th row of the block's chunk; contiguous views
// (sn = HW * sp, every BatchNorm) take 4 rows per iteration so 4 (MODE 2: 12) loads are in flight.
// T: element type of the maps v, dy, y (fp32 or bf16); sums in fp32.
// eval-mode 1 / sqrt(running_var + eps), correctly rounded (the same bits in every apply kernel)
__device__ __forceinline__ float bn_eval_rstd(float rv, float eps) {
#pragma clang fp contract(off)
  return __fdiv_rn(1.0f, __fsqrt_rn(rv + eps));
}

// dx of the BatchNorm backward at one element, rounding pinned (no contraction): the per-iteration and the
// channel-stationary kernels give the same bits however the compiler schedules or hoists the per-channel terms
__device__ __forceinline__ float bn_bwd_dx(float x, float g, float mu, float rs, float ga, float s0, float s1,
                                           float inv) {
#pragma clang fp contract(off)
  const float xh = (x - mu) * rs;
  const float t = (g - s0 * inv) - (xh * s1) * inv;
  return (rs * ga) * t;
}

// REBUILD (MODE 2, relu): the mask rebuilt from x with gamma / beta (bn_relu_live), y not read
// sdy (MODE 2): dy's own row stride, row r at dy + r * sdy (densenet.hip's strided backward); 0: dy laid out as v
template <int MODE, int VEC, typename T = float, bool REBUILD = false>
__global__ __launch_bounds__(256) void chan_partial_kernel(const T* __restrict__ v, RowMap rm, int rows, int C,
                                                           int rows_per, const float* __restrict__ mean,
                                                           const float* __restrict__ rstd, const T* __restrict__ dy,
                                                           const T* __restrict__ y, int relu,
                                                           float* __restrict__ partial,
                                                           const float* __restrict__ gamma = nullptr,
                                                           const float* __restrict__ beta = nullptr, long sdy = 0) {
  __shared__ float red[256 * VEC];
  __shared__ float red2[MODE == 2 ? 256 * VEC : 1];
  const int CV = C / VEC;
  const int cpp = CV < 256 ? CV : 256;  // vector columns per pass
  const int rp = 256 / cpp;             // row lanes
  const int t = threadIdx.x, cc = t % cpp, rl = t / cpp;
  const int r0 = blockIdx.x * rows_per, r1 = min(r0 + rows_per, rows);
  const bool contig = rm.sn == (long)rm.HW * rm.sp;
  for (int c0 = 0; c0 < CV; c0 += cpp) {
    const int cv = c0 + cc, c = cv * VEC;
    float s[VEC], s2[VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) s[j] = s2[j] = 0.f;
    if (rl < rp && cv < CV) {
      float mu[VEC], rs[VEC], ga[VEC], be[VEC];
#pragma unroll
      for (int j = 0; j < VEC; ++j) {
        mu[j] = MODE >= 1 ? mean[c + j] : 0.f;
        rs[j] = MODE == 2 ? rstd[c + j] : 0.f;
        if constexpr (REBUILD) {
          ga[j] = gamma[c + j];
          be[j] = beta[c + j];
        }
      }
      auto acc = [&](long o, int row) {
        float a[VEC];
        ldv<VEC>(v + o, a);
        if constexpr (MODE == 0) {
#pragma unroll
          for (int j = 0; j < VEC; ++j) s[j] += a[j];
        } else if constexpr (MODE == 1) {
#pragma unroll
          for (int j = 0; j < VEC; ++j) {
            const float d = a[j] - mu[j];
            s[j] = fmaf(d, d, s[j]);
          }
        } else {
          float gd[VEC], yy[VEC];
          ldv<VEC>(dy + (sdy ? (long)row * sdy + c : o), gd);
          if (!REBUILD && relu) ldv<VEC>(y + o, yy);
#pragma unroll
          for (int j = 0; j < VEC; ++j) {
            float gg;
            if constexpr (REBUILD) gg = bn_relu_live<T>(a[j], mu[j], rs[j], ga[j], be[j]) ? gd[j] : 0.f;
            else gg = (relu && !(yy[j] > 0.f)) ? 0.f : gd[j];
            s[j] += gg;
            s2[j] = fmaf(gg, (a[j] - mu[j]) * rs[j], s2[j]);
          }
        }
      };
      int r = r0 + rl;
      if (contig) {
        for (; r + 3 * rp < r1; r += 4 * rp) {
          acc((long)r * rm.sp + c, r);
          acc((long)(r + rp) * rm.sp + c, r + rp);
          acc((long)(r + 2 * rp) * rm.sp + c, r + 2 * rp);
          acc((long)(r + 3 * rp) * rm.sp + c, r + 3 * rp);
        }
        for (; r < r1; r += rp) acc((long)r * rm.sp + c, r);
      } else {
        int n = r / rm.HW, p = r - n * rm.HW;
        for (; r < r1; r += rp) {
          acc((long)n * rm.sn + (long)p * rm.sp + c, r);
          p += rp;
          while (p >= rm.HW) {
            p -= rm.HW;
            ++n;
          }
        }
      }
    }
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      red[t * VEC + j] = s[j];
      if constexpr (MODE == 2) red2[t * VEC + j] = s2[j];
    }
    __syncthreads();
    for (int q = t; q < cpp * VEC && c0 * VEC + q < C; q += 256) {
      const int col = q / VEC, j = q % VEC;
      float a = 0.f, b = 0.f;
      for (int l = 0; l < rp; ++l) {
        a += red[(l * cpp + col) * VEC + j];
        if constexpr (MODE == 2) b += red2[(l * cpp + col) * VEC + j];
      }
      partial[(long)blockIdx.x * (MODE == 2 ? 2 * C : C) + c0 * VEC + q] = a;
      if constexpr (MODE == 2) partial[(long)blockIdx.x * 2 * C + C + c0 * VEC + q] = b;
    }
    __syncthreads();
  }
}

// Second pass over the partials P[G][ncols]: 16 columns x 16 block lanes per workgroup, lanes
// summed in a fixed order (deterministic).  FIN selects what the column sum s becomes:
//   0  out[c] (+)= s                                        (bias gradients)
//   1  out[c] = s / rows                                    (BatchNorm batch mean)
//   2  out[c] = 1 / sqrt(s / rows + eps); running stats <- (1 - m) r + m (mean, s / (rows - 1))
//   3  out3[c] = s (when given); c < half: out[c] (+)= s, else out2[c - half] (+)= s
struct ChanFin {
  float *out, *out2, *out3;
  const float* mean;
  float *run_mean, *run_var;
  float eps, momentum;
  int rows, half, accumulate;
  int64_t* nbt = nullptr;  // FIN 2: num_batches_tracked += 1 by one thread of the launch
};
template <int FIN>
__global__ __launch_bounds__(256) void chan_final_kernel(const float* __restrict__ P, int G, int ncols, ChanFin f) {
  __shared__ float red[16][17];
  const int t = threadIdx.x, cl = t & 15, gl = t >> 4;
  const int c = blockIdx.x * 16 + cl;
  float s = 0.f;
  // unrolled: a lane's (up to 64) partial loads are issued ahead of its in-order adds (same sum,
  // bit for bit); the rolled loop paid one L2-miss latency per partial (16-20 us per launch)
  if (c < ncols) {
#pragma unroll 16
    for (int gI = gl; gI < G; gI += 16) s += P[(long)gI * ncols + c];
  }
  red[gl][cl] = s;
  __syncthreads();
  if (gl != 0 || c >= ncols) return;
  s = 0.f;
#pragma unroll
  for (int l = 0; l < 16; ++l) s += red[l][cl];
  if constexpr (FIN == 0) {
    f.out[c] = f.accumulate ? f.out[c] + s : s;
  } else if constexpr (FIN == 1) {
    f.out[c] = s / (float)f.rows;
  } else if constexpr (FIN == 2) {
    if (c == 0 && f.nbt) *f.nbt += 1;
    const float var = s / (float)f.rows;
    f.out[c] = 1.0f / sqrtf(var + f.eps);
    if (f.run_mean) {
      const float unb = f.rows > 1 ? s / (float)(f.rows - 1) : var;
      f.run_mean[c] = (1.f - f.momentum) * f.run_mean[c] + f.momentum * f.mean[c];
      f.run_var[c] = (1.f - f.momentum) * f.run_var[c] + f.momentum * unb;
    }
  } else {
    if (f.out3) f.out3[c] = s;
    float* o = c < f.half ? f.out + c : f.out2 + (c - f.half);
    *o = f.accumulate ? *o + s : s;
  }
}

inline int chan_groups(int rows) { return rows < 64 * 1024 ? (rows + 63) / 64 : 1024; }

// Batch statistics from per-block partials P[b][0][c] = block sum, P[b][1][c] = block M2 over blocks of
// `bsz` rows (the last one rows - (nblk-1) bsz), block b at P + b stride 2 PC (PC = the partials' channel count,
// >= C): mean = sum / n, M2 = sum_b M2_b + n_b (mean_b - mean)^2 (Chan et al.).  64 channels x 4 block lanes per workgroup, lanes
// combined in a fixed order.  !FINAL: workgroup y combines blocks [y G, y G + G) and writes the group's
// (sum, M2) over its first block's slot (read only by this workgroup, before its last barrier) -- the
// first of two levels, so no thread walks more than ~G / 4 blocks at any pixel count.
template <bool FINAL>
__global__ __launch_bounds__(256) void bn_stats_from_partials_kernel(float* __restrict__ P, int nblk, int bsz,
                                                                     int stride, int G, int rows, int C, int PC,
                                                                     float eps,
                                                                     float momentum, float* __restrict__ mean,
                                                                     float* __restrict__ rstd,
                                                                     float* __restrict__ run_mean,
                                                                     float* __restrict__ run_var,
                                                                     int64_t* __restrict__ nbt,
                                                                     float* __restrict__ m2o = nullptr) {
  __shared__ float red[4][64];
  if (FINAL && nbt && blockIdx.x == 0 && threadIdx.x == 0) *nbt += 1;  // num_batches_tracked (FINAL: one launch)
  const int cl = threadIdx.x & 63, bl = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + cl;
  const bool ok = c < C;
  const int b0 = blockIdx.y * G, b1 = min(nblk, b0 + G);
  const long bs = (long)stride * 2 * PC;
  const int rows_y = min(rows - b0 * bsz, (b1 - b0) * bsz);
  float s = 0.f;
  if (ok)
    for (int b = b0 + bl; b < b1; b += 4) s += P[b * bs + c];
  red[bl][cl] = s;
  __syncthreads();
  const float sum = (red[0][cl] + red[1][cl]) + (red[2][cl] + red[3][cl]);
  const float mu = sum / (float)rows_y;
  __syncthreads();
  float m2 = 0.f;
  if (ok)
    for (int b = b0 + bl; b < b1; b += 4) {
      const float nb = (float)(b + 1 < nblk ? bsz : rows - (nblk - 1) * bsz);
      const float d = P[b * bs + c] / nb - mu;
      m2 += P[b * bs + PC + c] + nb * d * d;
    }
  red[bl][cl] = m2;
  __syncthreads();
  if (bl != 0 || !ok) return;
  const float M2 = (red[0][cl] + red[1][cl]) + (red[2][cl] + red[3][cl]);
  if constexpr (!FINAL) {
    P[b0 * bs + c] = sum;
    P[b0 * bs + PC + c] = M2;
  } else {
    const float var = M2 / (float)rows;
    mean[c] = mu;
    rstd[c] = 1.0f / sqrtf(var + eps);
    if (m2o) m2o[c] = M2;  // the centred square sum itself (densenet.hip: the running update comes later)
    if (!run_mean) return;
    const float unb = rows > 1 ? M2 / (float)(rows - 1) : var;
    run_mean[c] = (1.f - momentum) * run_mean[c] + momentum * mu;
    run_var[c] = (1.f - momentum) * run_var[c] + momentum * unb;
  }
}

}  // namespace
