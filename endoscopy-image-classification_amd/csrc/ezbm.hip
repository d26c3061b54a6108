// EZBM stage 2 on the MI355X (gfx950): the classifier head `fc` trained on class-balanced mixes of the stored
// stage-1 features (code/ezbm.py:133-182, EmbFeatEZBM code/dataset.py:135-175).  fp32, no atomics (repeated
// launches give the same bits), every output entry written.
//
//  es_ezbm_sample_mix      one launch draws (or replays) a batch of n (row, dual) pairs from the feature bank
//                          and writes X = [mem[idx]; lam mem[idx] + (1 - lam) mem[dual]] with its targets
//  es_bn1d_groups_fwd/bwd  BatchNorm1d (train) over G consecutive groups of n rows, each with its own batch
//                          statistics, one set of weights and one gradient: fc(inputs) and fc(mix) as one pass
//  es_ezbm_ce_fwd_bwd      l_o + lambda_c l_s on the [2n, C] logits and its gradient
#include "common.h"

namespace {

// splitmix64 of (seed, counter): the hash of es_dropout_keep (comatch.hip), counter = offset + element index
__device__ __forceinline__ unsigned long long ezbm_hash(unsigned long long seed, unsigned long long counter) {
  unsigned long long z = seed + 0x9E3779B97F4A7C15ull * (counter + 1ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z ^= z >> 31;
  return z;
}

// a uniform member of class c's CSR range; -1 for an empty class (the host refuses those before any launch) or
// a range outside cls_idx's N entries
__device__ __forceinline__ int ezbm_member(const int* __restrict__ cls_off, const int* __restrict__ cls_idx, int N,
                                           int c, unsigned long long z) {
  const int lo = cls_off[c], m = cls_off[c + 1] - lo;
  if (m <= 0 || lo < 0 || lo > N - m) return -1;
  return cls_idx[lo + (int)(((z >> 40) * (unsigned long long)m) >> 24)];
}

// lam * a + oml * b as torch forms it in fp32: two rounded products, one rounded sum.  HIP's __fmul_rn /
// __fadd_rn are plain operators that the compiler may contract into an fma (the library is built with
// contraction on), so contraction is switched off for these three operations themselves.
__device__ __forceinline__ float ezbm_mix_rn(float lam, float a, float oml, float b) {
#pragma clang fp contract(off)
  const float p = lam * a;
  const float q = oml * b;
  return p + q;
}

constexpr int MIX_WAVES = 4;

// One wave per batch row (every lane computes the same draw), lanes strided over the D columns.  A row index
// outside [0, N) -- a bad replay index, an empty class -- reads nothing: its X rows are NaN, its target -1; a
// stored target outside [0, C) gives lam = NaN (no lam_table read).
__global__ __launch_bounds__(MIX_WAVES * 64) void ezbm_sample_mix_kernel(
    const float* __restrict__ mem, int ldm, const int64_t* __restrict__ mem_y, int N, int D, int C,
    const int* __restrict__ cls_off, const int* __restrict__ cls_idx, const float* __restrict__ cdf,
    const float* __restrict__ lam_table, unsigned long long seed, unsigned long long offset,
    const int* __restrict__ idx_in, const int* __restrict__ dual_in, int n, float* __restrict__ X, int ldx,
    int64_t* __restrict__ t_out, int64_t* __restrict__ td_out, float* __restrict__ lam_out, int* __restrict__ idx_out,
    int* __restrict__ dual_out) {
  const int i = blockIdx.x * MIX_WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (i >= n) return;  // wave-uniform
  int a, b;
  if (idx_in) {
    a = idx_in[i];
    b = dual_in[i];
  } else {
    const unsigned long long c0 = offset + 4ull * (unsigned long long)i;
    const int ca = (int)(((ezbm_hash(seed, c0) >> 40) * (unsigned long long)C) >> 24);
    a = ezbm_member(cls_off, cls_idx, N, ca, ezbm_hash(seed, c0 + 1ull));
    const float u = (float)(ezbm_hash(seed, c0 + 2ull) >> 40) * (1.0f / 16777216.0f);
    int cb = C - 1;
    for (int c = 0; c < C; ++c)
      if (u < cdf[c]) {
        cb = c;
        break;
      }
    b = ezbm_member(cls_off, cls_idx, N, cb, ezbm_hash(seed, c0 + 3ull));
  }
  const bool ok = (unsigned)a < (unsigned)N && (unsigned)b < (unsigned)N;
  const float nan = __int_as_float(0x7fc00000);
  const long long ta = ok ? (long long)mem_y[a] : -1ll, tb = ok ? (long long)mem_y[b] : -1ll;
  const bool tok = ok && (unsigned long long)ta < (unsigned long long)C && (unsigned long long)tb < (unsigned long long)C;
  const float lam = tok ? lam_table[(int)ta * C + (int)tb] : nan;
  const float oml = 1.0f - lam;
  float* xo = X + (size_t)i * ldx;
  float* xs = X + (size_t)(n + i) * ldx;
  if (ok) {
    const float* ra = mem + (size_t)a * ldm;
    const float* rb = mem + (size_t)b * ldm;
    for (int k = lane; k < D; k += 64) {
      const float va = ra[k];
      xo[k] = va;
      xs[k] = ezbm_mix_rn(lam, va, oml, rb[k]);  // torch's fp32 `lam * inputs + (1 - lam) * inputs_dual`
    }
  } else {
    for (int k = lane; k < D; k += 64) xo[k] = xs[k] = nan;
  }
  if (lane == 0) {
    t_out[i] = ta;
    td_out[i] = tb;
    lam_out[i] = lam;
    idx_out[i] = a;
    dual_out[i] = b;
  }
}

// bn1d_fwd_kernel's train branch (comatch.hip) once per group, in group order: one workgroup per feature, the
// same strides, reductions and running-buffer update, so G = 1 gives es_bn1d_fwd's bits.
__global__ __launch_bounds__(256) void bn1d_groups_fwd_kernel(const float* __restrict__ U, int ldu,
                                                              const float* __restrict__ gamma,
                                                              const float* __restrict__ beta, float* running_mean,
                                                              float* running_var, long long* nbt, float momentum,
                                                              float eps, float* __restrict__ Y, int ldy,
                                                              float* __restrict__ xhat, float* __restrict__ rstd_out,
                                                              int n, int G, int F) {
  __shared__ float red[256];
  const int f = blockIdx.x, t = threadIdx.x;
  const float g = gamma[f], bt = beta[f];
  for (int grp = 0; grp < G; ++grp) {
    const float* Ug = U + (size_t)grp * n * ldu;
    float s = 0.f;
    for (int i = t; i < n; i += blockDim.x) s += Ug[(size_t)i * ldu + f];
    red[t] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
      if (t < o) red[t] += red[t + o];
      __syncthreads();
    }
    const float mean = red[0] / n;
    __syncthreads();
    float ss = 0.f;
    for (int i = t; i < n; i += blockDim.x) {
      const float d = Ug[(size_t)i * ldu + f] - mean;
      ss += d * d;
    }
    red[t] = ss;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
      if (t < o) red[t] += red[t + o];
      __syncthreads();
    }
    const float var = red[0] / n;
    const float rstd = 1.0f / sqrtf(var + eps);
    if (t == 0) {
      running_mean[f] = (1.f - momentum) * running_mean[f] + momentum * mean;
      running_var[f] = (1.f - momentum) * running_var[f] + momentum * (n > 1 ? var * n / (n - 1) : var);
      if (f == 0 && nbt) *nbt += 1;
      rstd_out[(size_t)grp * F + f] = rstd;
    }
    float* Yg = Y + (size_t)grp * n * ldy;
    float* xg = xhat + (size_t)grp * n * F;
    for (int i = t; i < n; i += blockDim.x) {
      const float xh = (Ug[(size_t)i * ldu + f] - mean) * rstd;
      xg[(size_t)i * F + f] = xh;
      Yg[(size_t)i * ldy + f] = xh * g + bt;
    }
    __syncthreads();  // red[0] (var) is read above; the next group writes red again
  }
}

// bn1d_bwd_kernel (comatch.hip) per group with the group's own sums; dgamma / dbeta = the groups' sums added in
// group order, plain overwrite.
__global__ __launch_bounds__(256) void bn1d_groups_bwd_kernel(const float* __restrict__ dY, int lddy,
                                                              const float* __restrict__ xhat,
                                                              const float* __restrict__ rstd,
                                                              const float* __restrict__ gamma, float* __restrict__ dU,
                                                              int lddu, float* __restrict__ dgamma,
                                                              float* __restrict__ dbeta, int n, int G, int F) {
  __shared__ float r1[256], r2[256];
  const int f = blockIdx.x, t = threadIdx.x;
  float dg = 0.f, db = 0.f;
  for (int grp = 0; grp < G; ++grp) {
    const float* dYg = dY + (size_t)grp * n * lddy;
    const float* xg = xhat + (size_t)grp * n * F;
    float* dUg = dU + (size_t)grp * n * lddu;
    float s1 = 0.f, s2 = 0.f;
    for (int i = t; i < n; i += blockDim.x) {
      const float g = dYg[(size_t)i * lddy + f];
      s1 += g;
      s2 += g * xg[(size_t)i * F + f];
    }
    r1[t] = s1;
    r2[t] = s2;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
      if (t < o) {
        r1[t] += r1[t + o];
        r2[t] += r2[t + o];
      }
      __syncthreads();
    }
    const float sdy = r1[0], sdyx = r2[0];
    dg = grp == 0 ? sdyx : dg + sdyx;
    db = grp == 0 ? sdy : db + sdy;
    const float k = gamma[f] * rstd[(size_t)grp * F + f], m1 = sdy / n, m2 = sdyx / n;
    for (int i = t; i < n; i += blockDim.x)
      dUg[(size_t)i * lddu + f] = k * (dYg[(size_t)i * lddy + f] - m1 - xg[(size_t)i * F + f] * m2);
    __syncthreads();  // r1[0] / r2[0] are read above; the next group writes them again
  }
  if (t == 0) {
    dgamma[f] = dg;
    dbeta[f] = db;
  }
}

__device__ __forceinline__ float ezbm_block_sum(float v, float* red) {
  v = warp_sum(v);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) red[w] = v;
  __syncthreads();
  float s = 0.f;
  for (int i = 0; i < (int)(blockDim.x >> 6); ++i) s += red[i];
  return s;
}

// max and log(sum exp(l - max)) of a row
__device__ __forceinline__ void ezbm_row_lse(const float* __restrict__ r, int C, float& mx, float& lg) {
  mx = -INFINITY;
  for (int c = 0; c < C; ++c) mx = fmaxf(mx, r[c]);
  float se = 0.f;
  for (int c = 0; c < C; ++c) se += expf(r[c] - mx);
  lg = logf(se);
}

// One workgroup, a thread per pair i (rows i and n + i).  CE(r, y) = log sum exp(r - max) - (r[y] - max).  The
// three sums run per thread in row order, then lanes, then waves: a fixed order.
__global__ __launch_bounds__(256) void ezbm_ce_kernel(const float* __restrict__ l, int ldl,
                                                      const int64_t* __restrict__ t, const int64_t* __restrict__ td,
                                                      int n, int C, float lambda_c, float grad_scale,
                                                      float* __restrict__ dl, int lddl, float* __restrict__ out) {
  __shared__ float red[16];
  float s_o = 0.f, s_t = 0.f, s_d = 0.f;
  const float ko = grad_scale / (float)n, ks = grad_scale * lambda_c / (float)n;
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    const float* ro = l + (size_t)i * ldl;
    const float* rs = l + (size_t)(n + i) * ldl;
    float* go = dl + (size_t)i * lddl;
    float* gs = dl + (size_t)(n + i) * lddl;
    const long long y = (long long)t[i], yd = (long long)td[i];
    if ((unsigned long long)y >= (unsigned long long)C || (unsigned long long)yd >= (unsigned long long)C) {
      // invalid target: NaN loss, no gradient, no out-of-range read
      s_o += __int_as_float(0x7fc00000);
      for (int c = 0; c < C; ++c) go[c] = gs[c] = 0.f;
      continue;
    }
    const int yi = (int)y, ydi = (int)yd;
    float mx, lg;
    ezbm_row_lse(ro, C, mx, lg);
    s_o += lg - (ro[yi] - mx);
    for (int c = 0; c < C; ++c) go[c] = ko * (expf(ro[c] - mx - lg) - (c == yi ? 1.f : 0.f));
    ezbm_row_lse(rs, C, mx, lg);
    s_t += lg - (rs[yi] - mx);
    s_d += lg - (rs[ydi] - mx);
    for (int c = 0; c < C; ++c)
      gs[c] = ks * (expf(rs[c] - mx - lg) - (c == yi ? 0.5f : 0.f) - (c == ydi ? 0.5f : 0.f));
  }
  s_o = ezbm_block_sum(s_o, red);
  s_t = ezbm_block_sum(s_t, red);
  s_d = ezbm_block_sum(s_d, red);
  if (threadIdx.x == 0) {
    const float l_o = s_o / (float)n;
    const float l_s = 0.5f * (s_t / (float)n) + 0.5f * (s_d / (float)n);
    out[0] = l_o + lambda_c * l_s;
    out[1] = l_o;
    out[2] = l_s;
  }
}

}  // namespace

extern "C" {

int es_ezbm_sample_mix(const float* mem, int ldm, const int64_t* mem_y, int N, int D, int C, const int* cls_off,
                       const int* cls_idx, const float* cdf, const float* lam_table, unsigned long long seed,
                       unsigned long long offset, const int* idx_in, const int* dual_in, int n, float* X, int ldx,
                       int64_t* t, int64_t* td, float* lam, int* idx, int* dual, hipStream_t stream) {
  if (n < 1 || n > 0x3fffffff || N < 1 || N >= (1 << 24) || D < 1 || D > 2048 || C < 1 || C > 64 || ldm < D || ldx < D)
    return ES_BAD_SHAPE;
  if (!mem || !mem_y || !lam_table || !X || !t || !td || !lam || !idx || !dual) return ES_BAD_ARG;
  if ((idx_in == nullptr) != (dual_in == nullptr)) return ES_BAD_ARG;  // replay needs both
  if (!idx_in && (!cls_off || !cls_idx || !cdf)) return ES_BAD_ARG;    // a draw needs the class table and the CDF
  hipLaunchKernelGGL(ezbm_sample_mix_kernel, (n + MIX_WAVES - 1) / MIX_WAVES, MIX_WAVES * 64, 0, stream, mem, ldm,
                     mem_y, N, D, C, cls_off, cls_idx, cdf, lam_table, seed, offset, idx_in, dual_in, n, X, ldx, t, td,
                     lam, idx, dual);
  return hipGetLastError() == hipSuccess ? ES_OK : ES_HIP_ERROR;
}

int es_bn1d_groups_fwd(const float* U, int ldu, const float* gamma, const float* beta, float* running_mean,
                       float* running_var, void* num_batches_tracked, float momentum, float eps, float* Y, int ldy,
                       float* xhat, float* rstd, int n, int G, int F, hipStream_t stream) {
  if (n < 2 || G < 1 || F < 1 || ldu < F || ldy < F || (long long)n * G > 0x7fffffffll) return ES_BAD_SHAPE;
  if (!U || !gamma || !beta || !running_mean || !running_var || !Y || !xhat || !rstd) return ES_BAD_ARG;
  hipLaunchKernelGGL(bn1d_groups_fwd_kernel, F, 256, 0, stream, U, ldu, gamma, beta, running_mean, running_var,
                     (long long*)num_batches_tracked, momentum, eps, Y, ldy, xhat, rstd, n, G, F);
  return hipGetLastError() == hipSuccess ? ES_OK : ES_HIP_ERROR;
}

int es_bn1d_groups_bwd(const float* dY, int lddy, const float* xhat, const float* rstd, const float* gamma, float* dU,
                       int lddu, float* dgamma, float* dbeta, int n, int G, int F, hipStream_t stream) {
  if (n < 2 || G < 1 || F < 1 || lddy < F || lddu < F || (long long)n * G > 0x7fffffffll) return ES_BAD_SHAPE;
  if (!dY || !xhat || !rstd || !gamma || !dU || !dgamma || !dbeta) return ES_BAD_ARG;
  hipLaunchKernelGGL(bn1d_groups_bwd_kernel, F, 256, 0, stream, dY, lddy, xhat, rstd, gamma, dU, lddu, dgamma, dbeta,
                     n, G, F);
  return hipGetLastError() == hipSuccess ? ES_OK : ES_HIP_ERROR;
}

int es_ezbm_ce_fwd_bwd(const float* logits, int ldl, const int64_t* t, const int64_t* td, int n, int C, float lambda_c,
                       float grad_scale, float* dlogits, int lddl, float* out, hipStream_t stream) {
  if (n < 1 || n > 0x3fffffff || C < 1 || ldl < C || lddl < C) return ES_BAD_SHAPE;
  if (!logits || !t || !td || !dlogits || !out) return ES_BAD_ARG;
  hipLaunchKernelGGL(ezbm_ce_kernel, 1, 256, 0, stream, logits, ldl, t, td, n, C, lambda_c, grad_scale, dlogits, lddl,
                     out);
  return hipGetLastError() == hipSuccess ? ES_OK : ES_HIP_ERROR;
}

}  // extern "C"
