// Fused FixMatch loss kernels: forward value AND d(loss)/d(logits) in one launch (gfx950).
//
//  es_fm_consistency_fwd_bwd  code/loss.py:126-164 (consistency_loss, name='ce', hard labels):
//      p = softmax(detach(l_w)); (max_p, idx) = max(p, -1)   [first index on ties]
//      mask = (max_p >= tau)                                 [inclusive]
//      loss = mean_i( CE(l_s[i], idx[i]) * mask[i] ),  mask_mean = mean(mask)   (T unused)
//      d loss / d l_s[i][c] = mask[i] * (softmax(l_s[i])_c - [c == idx[i]]) * grad_scale
//  es_poly_ce_fwd_bwd         code/loss.py:103-114,308-364 (PolyLoss, softmax=True, epsilon=2):
//      loss = mean_i( w[y_i] * CE_i + eps * (1 - p_i[y_i]) )   (plain mean, not weight-normalised)
//      d/d l[i][c] = grad_scale * (w[y_i] + eps * p_i[y_i]) * (p_i[c] - [c == y_i])
//  es_triplet_fwd_bwd         code/loss.py:170-190 (TripletLoss, alpha = 0.7) on z = [anchors; positives; negatives]
//  es_softmax_predict         code/supervised.py:258-266 (inference: argmax, max probability, thresholded label)
//  es_margin_softmax_fwd_bwd  code/loss.py:228-266 (AngularPenaltySMLoss: normalise, fc, margin, softmax) with
//      d/dx, d/dW, d/db -- its own two kernels, described where they stand
// The logits are tiny ([448,23] / [64,23]); one workgroup handles all rows, staging each row's
// logits in registers, and emits int32 pseudo-labels, the uint8 mask, per-row losses and the two
// means -- no host sync and no intermediate tensors.
#include "common.h"

namespace {

constexpr int MAXC = 64;

__device__ __forceinline__ float block_sum(float v, float* red) {
  v = warp_sum(v);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) red[w] = v;
  __syncthreads();
  float s = 0.f;
  for (int i = 0; i < (int)(blockDim.x >> 6); ++i) s += red[i];
  return s;
}

// The class index of a 64-bit target, or -1 where the value itself lies outside [0, C): the range check comes
// before the narrowing, so 2^32 + 3 is invalid and not class 3.
__device__ __forceinline__ int target_index(int64_t y64, int C) { return y64 >= 0 && y64 < C ? (int)y64 : -1; }

__global__ __launch_bounds__(256) void fm_consistency_kernel(const float* __restrict__ lw, int ldw,
                                                             const float* __restrict__ ls, int lds_, int n, int C,
                                                             float tau, float grad_scale, int* __restrict__ pl,
                                                             uint8_t* __restrict__ mask_out,
                                                             float* __restrict__ row_loss, float* __restrict__ dls,
                                                             int lddls, float* __restrict__ out) {
  __shared__ float red[16];
  float sum_loss = 0.f, sum_mask = 0.f;
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    // pseudo-label from the weak view (logits re-read from L1 instead of a private array)
    const float* wr = lw + (size_t)i * ldw;
    const float* sr = ls + (size_t)i * lds_;
    float mx = -INFINITY;
    for (int c = 0; c < C; ++c) mx = fmaxf(mx, wr[c]);
    float se = 0.f;
    for (int c = 0; c < C; ++c) se += __expf(wr[c] - mx);
    const float inv = 1.0f / se;
    float pmax = -1.f;
    int idx = 0;
    for (int c = 0; c < C; ++c) {
      const float p = __expf(wr[c] - mx) * inv;
      if (p > pmax) {
        pmax = p;
        idx = c;
      }
    }
    const float m = pmax >= tau ? 1.f : 0.f;
    // CE of the strong view against idx
    float mxs = -INFINITY;
    for (int c = 0; c < C; ++c) mxs = fmaxf(mxs, sr[c]);
    float ses = 0.f;
    for (int c = 0; c < C; ++c) ses += __expf(sr[c] - mxs);
    const float lse = mxs + __logf(ses);
    const float ce = lse - sr[idx];
    const float rl = ce * m;
    const float invs = 1.0f / ses;
    for (int c = 0; c < C; ++c) {
      const float p = __expf(sr[c] - mxs) * invs;
      dls[(size_t)i * lddls + c] = m * (p - (c == idx ? 1.f : 0.f)) * grad_scale;
    }
    if (pl) pl[i] = idx;
    if (mask_out) mask_out[i] = (uint8_t)m;
    if (row_loss) row_loss[i] = rl;
    sum_loss += rl;
    sum_mask += m;
  }
  sum_loss = block_sum(sum_loss, red);
  sum_mask = block_sum(sum_mask, red);
  if (threadIdx.x == 0) {
    out[0] = sum_loss / (float)n;
    out[1] = sum_mask / (float)n;
  }
}

__global__ __launch_bounds__(256) void poly_ce_kernel(const float* __restrict__ l, int ldl,
                                                      const int64_t* __restrict__ y, const float* __restrict__ w,
                                                      int n, int C, float eps, float grad_scale,
                                                      float* __restrict__ dl, int lddl, float* __restrict__ out) {
  __shared__ float red[16];
  float sum = 0.f;
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    const float* lr = l + (size_t)i * ldl;
    float mx = -INFINITY;
    for (int c = 0; c < C; ++c) mx = fmaxf(mx, lr[c]);
    float se = 0.f;
    for (int c = 0; c < C; ++c) se += __expf(lr[c] - mx);
    const float lse = mx + __logf(se);
    const int yi = target_index(y[i], C);
    if ((unsigned)yi >= (unsigned)C) {  // invalid target: NaN loss, no gradient, no out-of-range read
      sum += __int_as_float(0x7fc00000);
      for (int c = 0; c < C; ++c) dl[(size_t)i * lddl + c] = 0.f;
      continue;
    }
    const float wy = w ? w[yi] : 1.f;
    const float py = __expf(lr[yi] - lse);
    sum += wy * (lse - lr[yi]) + eps * (1.f - py);
    const float coef = grad_scale * (wy + eps * py);
    for (int c = 0; c < C; ++c) {
      const float p = __expf(lr[c] - lse);
      dl[(size_t)i * lddl + c] = coef * (p - (c == yi ? 1.f : 0.f));
    }
  }
  sum = block_sum(sum, red);
  if (threadIdx.x == 0) out[0] = sum / (float)n;
}

// F.cross_entropy(logits, y, weight=w, reduction='mean') = sum_i w[y_i] l_i / sum_i w[y_i]
// (code/loss.py:118, the SemiFormer heads' loss, code/semiformer.py:125-126); one workgroup.
__global__ __launch_bounds__(256) void ce_weighted_kernel(const float* __restrict__ l, int ldl,
                                                          const int64_t* __restrict__ y, const float* __restrict__ w,
                                                          const float* __restrict__ wsum_global, int n, int C,
                                                          float grad_scale, float* __restrict__ dl, int lddl,
                                                          float* __restrict__ out) {
  __shared__ float red[16];
  float ws = 0.f;
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    const int yi = target_index(y[i], C);
    ws += (unsigned)yi >= (unsigned)C ? __int_as_float(0x7fc00000) : (w ? w[yi] : 1.f);
  }
  float W = block_sum(ws, red);
  __syncthreads();
  if (wsum_global) W = *wsum_global;  // the whole batch's weight sum over every rank (data-parallel step)
  const float invW = 1.0f / W;
  float sum = 0.f;
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    const float* lr = l + (size_t)i * ldl;
    float mx = -INFINITY;
    for (int c = 0; c < C; ++c) mx = fmaxf(mx, lr[c]);
    float se = 0.f;
    for (int c = 0; c < C; ++c) se += __expf(lr[c] - mx);
    const float lse = mx + __logf(se);
    const int yi = target_index(y[i], C);
    if ((unsigned)yi >= (unsigned)C) {  // invalid target: NaN loss (via the weight sum), no gradient
      for (int c = 0; c < C; ++c) dl[(size_t)i * lddl + c] = 0.f;
      continue;
    }
    const float wy = w ? w[yi] : 1.f;
    sum += wy * (lse - lr[yi]);
    const float coef = grad_scale * wy * invW;
    for (int c = 0; c < C; ++c) {
      const float p = __expf(lr[c] - lse);
      dl[(size_t)i * lddl + c] = coef * (p - (c == yi ? 1.f : 0.f));
    }
  }
  sum = block_sum(sum, red);
  if (threadIdx.x == 0) out[0] = sum * invW;
}

__global__ __launch_bounds__(256) void ce_weight_sum_kernel(const int64_t* __restrict__ y, const float* __restrict__ w,
                                                            int n, int C, float* __restrict__ out) {
  __shared__ float red[16];
  float ws = 0.f;
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    const int yi = target_index(y[i], C);
    ws += (unsigned)yi >= (unsigned)C ? __int_as_float(0x7fc00000) : (w ? w[yi] : 1.f);
  }
  ws = block_sum(ws, red);
  if (threadIdx.x == 0) out[0] = ws;
}

// TripletLoss (code/loss.py:170-190) on the L2-normalised embeddings, value and gradient; one workgroup,
// one wave per triplet (wave w takes triplets w, w + nw, ...).  Lanes stride the L columns twice: the
// squared distances, then -- the rows still in L1 -- the three gradient rows.  The four means are summed per
// wave in triplet order and across waves in wave order: no atomics, the same bits on every launch.
constexpr int TRIPLET_THREADS = 1024;

__global__ __launch_bounds__(TRIPLET_THREADS) void triplet_kernel(const float* __restrict__ z, int ldz, int bs, int L,
                                                                  float alpha, float grad_scale,
                                                                  float* __restrict__ dz, int lddz,
                                                                  float* __restrict__ out) {
  __shared__ float red[16];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
  float s_h = 0.f, s_p = 0.f, s_n = 0.f, s_act = 0.f;  // wave-uniform
  for (int i = w; i < bs; i += nw) {
    const float* za = z + (size_t)i * ldz;
    const float* zp = z + (size_t)(bs + i) * ldz;
    const float* zn = z + (size_t)(2 * bs + i) * ldz;
    float sp = 0.f, sn = 0.f;
    for (int k = lane; k < L; k += 64) {
      const float a = za[k], ep = a - zp[k], en = a - zn[k];
      sp = fmaf(ep, ep, sp);
      sn = fmaf(en, en, sn);
    }
    const float dp = sqrtf(warp_sum(sp)), dn = sqrtf(warp_sum(sn));
    const float h = dp - dn + alpha;
    const bool act = h > 0.f;  // h == 0 is inactive
    s_h += act ? h : 0.f;
    s_p += dp;
    s_n += dn;
    s_act += act ? 1.f : 0.f;
    // unit directions scaled by grad_scale; 0 at zero distance (torch.norm's backward) and for h <= 0
    const float cp = act && dp > 0.f ? grad_scale / dp : 0.f;
    const float cn = act && dn > 0.f ? grad_scale / dn : 0.f;
    float* ga = dz + (size_t)i * lddz;
    float* gp = dz + (size_t)(bs + i) * lddz;
    float* gn = dz + (size_t)(2 * bs + i) * lddz;
    for (int k = lane; k < L; k += 64) {
      const float a = za[k], up = (a - zp[k]) * cp, un = (a - zn[k]) * cn;
      ga[k] = up - un;
      gp[k] = -up;
      gn[k] = un;
    }
  }
  const float inv = 1.0f / (float)bs;
  s_h = block_sum(lane == 0 ? s_h : 0.f, red);
  s_p = block_sum(lane == 0 ? s_p : 0.f, red);
  s_n = block_sum(lane == 0 ? s_n : 0.f, red);
  s_act = block_sum(lane == 0 ? s_act : 0.f, red);
  if (threadIdx.x == 0) {
    out[0] = s_h * inv;
    out[1] = s_p * inv;
    out[2] = s_n * inv;
    out[3] = s_act * inv;
  }
}

// softmax argmax / confidence / thresholded label per row (code/supervised.py:238-268, inference): a thread
// per row, grid-stride over the rows.  conf = 1 / sum_c exp(l_c - max): the max's own probability.
__global__ __launch_bounds__(256) void softmax_predict_kernel(const float* __restrict__ l, int ldl, int n, int C,
                                                              float thres, int* __restrict__ pred,
                                                              float* __restrict__ conf, int* __restrict__ label) {
  const int stride = gridDim.x * blockDim.x;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const float* lr = l + (size_t)i * ldl;
    float mx = lr[0];
    int idx = 0;
    for (int c = 1; c < C; ++c) {
      const float v = lr[c];
      if (v > mx) {  // strict: the first index on ties
        mx = v;
        idx = c;
      }
    }
    float se = 0.f;
    for (int c = 0; c < C; ++c) se += __expf(lr[c] - mx);
    const float p = 1.0f / se;
    if (pred) pred[i] = idx;
    if (conf) conf[i] = p;
    if (label) label[i] = p > thres ? idx : 0;
  }
}

// AngularPenaltySMLoss (code/loss.py:228-266), value and gradient, in two launches on one stream.
//  margin_rows_kernel    one workgroup of 4 waves per row i:
//      x^ = x / max(|x|, 1e-12) into LDS; z_c = x^ . W_c (+ b_c), a wave per class (lanes stride the columns,
//      wave sum); wave 0, lane c: v_c = num(t) at the target, s z_c elsewhere, lse by max subtraction,
//      g_c = d(-grad_scale w m L_i)/d z_c into the workspace; then every thread, for its columns,
//      dx^ = sum_c g_c W_c (class order) and dx through the normalisation.
//  margin_reduce_kernel  dW[c] = sum_i g[i][c] x^_i, a thread per (class, 4 columns), rows in order; db and the
//      loss sum by a wave each (lane l takes rows l, l + 64, ..., then the wave sum).
// No atomics, every sum in a fixed order: the same bits on every launch.
constexpr int MARGIN_THREADS = 256;
constexpr int MARGIN_MAXF = 2048;
enum { MARGIN_COSFACE = 0, MARGIN_ARCFACE = 1, MARGIN_SPHEREFACE = 2, MARGIN_ACLOSS = 3 };

struct MarginParams {
  int kind;
  float s, m, eps, lo, hi;  // lo, hi: the clamp range of the target cosine, -1 + eps and 1 - eps in fp32
  float cos_m, sin_m;  // arcface: cos(theta + m) = t cos m - sqrt(1 - t^2) sin m
  float sig1, inv_k;   // acloss g_theta: (1 + e^(-pi/2k)) / (1 - e^(-pi/2k)), 1 / k
  float grad_scale;
};

// num(t) and d num / d t; the clamp passes no gradient outside [lo, hi] (torch.clamp's backward)
__device__ __forceinline__ void margin_numerator(const MarginParams& P, float t, float& num, float& dnum) {
  if (P.kind == MARGIN_COSFACE) {
    num = P.s * (t - P.m);
    dnum = P.s;
    return;
  }
  const bool inside = t >= P.lo && t <= P.hi;
  const float tc = fminf(fmaxf(t, P.lo), P.hi);
  // 1 -+ tc: exact differences inside the range; at a clamped end the distance to +-1 is eps itself, which
  // fp32 cannot carry in tc (1 - 1e-7 rounds to 1 - 1.19e-7).  sq = sin(acos(tc)) > 0, theta = acos(tc)
  const float om = inside ? 1.0f - tc : (t > P.hi ? P.eps : 2.0f - P.eps);
  const float op = inside ? 1.0f + tc : (t > P.hi ? 2.0f - P.eps : P.eps);
  const float sq = sqrtf(om * op);
  float d;
  if (P.kind == MARGIN_ARCFACE) {
    num = P.s * (tc * P.cos_m - sq * P.sin_m);
    d = P.s * (P.cos_m + tc * P.sin_m / sq);
  } else if (P.kind == MARGIN_SPHEREFACE) {
    const float th = P.m * atan2f(sq, tc);
    num = P.s * cosf(th);
    d = P.s * P.m * sinf(th) / sq;
  } else {  // acloss: s g_theta(acos(tc) + m), g_theta(a) = sig1 (1 - e) / (1 + e), e = exp((a - pi/2) / k)
    const float e = expf((atan2f(sq, tc) + P.m - 1.57079632679489662f) * P.inv_k);
    num = P.s * P.sig1 * (1.0f - e) / (1.0f + e);
    d = P.s * P.sig1 * 2.0f * e * P.inv_k / ((1.0f + e) * (1.0f + e) * sq);
  }
  dnum = inside ? d : 0.f;
}

__global__ __launch_bounds__(MARGIN_THREADS) void margin_rows_kernel(
    const float* __restrict__ x, int ldx, const float* __restrict__ W, const float* __restrict__ b,
    const int64_t* __restrict__ y, const float* __restrict__ cw, const float* __restrict__ mask, int F, int C,
    MarginParams P, float* __restrict__ dx, int lddx, float* __restrict__ G, float* __restrict__ inv_norm,
    float* __restrict__ ws_loss, float* __restrict__ row_loss) {
  __shared__ __attribute__((aligned(16))) float xs[MARGIN_MAXF];
  __shared__ float zs[MAXC], gs[MAXC], red[16];
  const int i = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int F4 = F >> 2;
  const f32x4* xr = (const f32x4*)(x + (size_t)i * ldx);
  float ss = 0.f;
  for (int k = tid; k < F4; k += MARGIN_THREADS) {
    const f32x4 v = xr[k];
    ss += v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3];
  }
  const float nrm = sqrtf(block_sum(ss, red));
  const float inv = 1.0f / fmaxf(nrm, 1e-12f);
  for (int k = tid; k < F4; k += MARGIN_THREADS) ((f32x4*)xs)[k] = xr[k] * inv;
  __syncthreads();
  for (int c = w; c < C; c += MARGIN_THREADS / 64) {
    const f32x4* wr = (const f32x4*)(W + (size_t)c * F);
    float acc = 0.f;
    for (int k = lane; k < F4; k += 64) {
      const f32x4 a = ((const f32x4*)xs)[k], q = wr[k];
      acc = fmaf(a[0], q[0], acc);
      acc = fmaf(a[1], q[1], acc);
      acc = fmaf(a[2], q[2], acc);
      acc = fmaf(a[3], q[3], acc);
    }
    acc = warp_sum(acc);
    if (lane == 0) zs[c] = acc + (b ? b[c] : 0.f);
  }
  __syncthreads();
  if (w == 0) {
    const int64_t y64 = y[i];
    const bool valid = y64 >= 0 && y64 < C;
    const int yi = valid ? (int)y64 : -1;
    const float wm = (valid && cw ? cw[yi] : 1.f) * (mask ? mask[i] : 1.f);
    float num = 0.f, dnum = 0.f;
    margin_numerator(P, zs[valid ? yi : 0], num, dnum);
    const bool tgt = lane == yi;
    const float v = lane < C ? (tgt ? num : P.s * zs[lane]) : -INFINITY;
    const float mx = warp_max(v);
    const float e = lane < C ? expf(v - mx) : 0.f;
    const float se = warp_sum(e);
    const float rest = warp_sum(tgt ? 0.f : e);  // 1 - p_target = rest / se, without the cancellation
    const float lse = mx + logf(se);
    const float coef = P.grad_scale * wm;
    float g = tgt ? -coef * (rest / se) * dnum : coef * P.s * (e / se);
    float rl = wm * (lse - num);
    if (!valid) {  // invalid target: NaN loss, no gradient, no out-of-range read
      g = 0.f;
      rl = __int_as_float(0x7fc00000);
    }
    if (lane < C) {
      gs[lane] = g;
      G[(size_t)i * C + lane] = g;
    }
    if (lane == 0) {
      inv_norm[i] = inv;
      ws_loss[i] = rl;
      if (row_loss) row_loss[i] = rl;
    }
  }
  __syncthreads();
  // at most MARGIN_MAXF / 4 / MARGIN_THREADS = 2 column groups per thread
  f32x4 acc[2];
  float dot = 0.f;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int k = tid + j * MARGIN_THREADS;
    acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (k < F4) {
      for (int c = 0; c < C; ++c) acc[j] += ((const f32x4*)(W + (size_t)c * F))[k] * gs[c];
      const f32x4 a = ((const f32x4*)xs)[k];
      dot += a[0] * acc[j][0] + a[1] * acc[j][1] + a[2] * acc[j][2] + a[3] * acc[j][3];
    }
  }
  dot = block_sum(dot, red);
  // F.normalize's backward: through x / |x| where |x| >= 1e-12, else through x / 1e-12 alone
  const float proj = nrm >= 1e-12f ? dot : 0.f;
  f32x4* dr = (f32x4*)(dx + (size_t)i * lddx);
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int k = tid + j * MARGIN_THREADS;
    if (k < F4) dr[k] = (acc[j] - ((const f32x4*)xs)[k] * proj) * inv;
  }
}

__global__ __launch_bounds__(64) void margin_reduce_kernel(const float* __restrict__ x, int ldx,
                                                           const float* __restrict__ G,
                                                           const float* __restrict__ inv_norm,
                                                           const float* __restrict__ ws_loss, int n, int F, int C,
                                                           float grad_scale, float* __restrict__ dW,
                                                           float* __restrict__ db, float* __restrict__ out) {
  const int c = blockIdx.y, lane = threadIdx.x;
  const int F4 = F >> 2, k = blockIdx.x * 64 + lane;
  if (k < F4) {
    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
    for (int i = 0; i < n; ++i)
      acc += ((const f32x4*)(x + (size_t)i * ldx))[k] * (G[(size_t)i * C + c] * inv_norm[i]);
    ((f32x4*)(dW + (size_t)c * F))[k] = acc;
  }
  if (blockIdx.x == 0) {
    if (db) {
      float sb = 0.f;
      for (int i = lane; i < n; i += 64) sb += G[(size_t)i * C + c];
      sb = warp_sum(sb);
      if (lane == 0) db[c] = sb;
    }
    if (c == 0) {
      float sl = 0.f;
      for (int i = lane; i < n; i += 64) sl += ws_loss[i];
      sl = warp_sum(sl);
      if (lane == 0) out[0] = grad_scale * sl;
    }
  }
}

}  // namespace

extern "C" {

// out[0] = weighted-mean CE (weights nullable -> plain mean); dl = grad_scale * d(out[0])/d logits
int es_ce_weighted_fwd_bwd(const float* logits, int ldl, const int64_t* targets, const float* weights, int n, int C,
                           float grad_scale, float* dlogits, int lddl, float* out, hipStream_t stream) {
  if (n <= 0 || C <= 0 || ldl < C || lddl < C) return ES_BAD_SHAPE;
  if (!logits || !targets || !dlogits || !out) return ES_BAD_ARG;
  hipLaunchKernelGGL(ce_weighted_kernel, 1, 256, 0, stream, logits, ldl, targets, weights, nullptr, n, C, grad_scale,
                     dlogits, lddl, out);
  return hipGetLastError() == hipSuccess ? ES_OK : ES_HIP_ERROR;
}

// out[0] = sum_i w[y_i] (the local weight sum of the weighted mean; weights nullable -> n)
int es_ce_weight_sum(const int64_t* targets, const float* weights, int n, int C, float* out, hipStream_t stream) {
  if (n <= 0 || C <= 0) return ES_BAD_SHAPE;
  if (!targets || !out) return ES_BAD_ARG;
  hipLaunchKernelGGL(ce_weight_sum_kernel, 1, 256, 0, stream, targets, weights, n, C, out);
  return hipGetLastError() == hipSuccess ? ES_OK : ES_HIP_ERROR;
}

// The data-parallel form: the rows are this rank's shard, *wsum_global the weight sum over every
// rank's rows (es_ce_weight_sum + a SUM all-reduce), so out[0] = this shard's share of the global
// weighted mean, sum_{i in shard} w l_i / W_global, and dl = grad_scale * d(out[0])/d logits.
int es_ce_weighted_fwd_bwd_global(const float* logits, int ldl, const int64_t* targets, const float* weights,
                                  const float* wsum_global, int n, int C, float grad_scale, float* dlogits, int lddl,
                                  float* out, hipStream_t stream) {
  if (n <= 0 || C <= 0 || ldl < C || lddl < C) return ES_BAD_SHAPE;
  if (!logits || !targets || !dlogits || !out || !wsum_global) return ES_BAD_ARG;
  hipLaunchKernelGGL(ce_weighted_kernel, 1, 256, 0, stream, logits, ldl, targets, weights, wsum_global, n, C,
                     grad_scale, dlogits, lddl, out);
  return hipGetLastError() == hipSuccess ? ES_OK : ES_HIP_ERROR;
}

// out[0] = loss (mean over n of masked CE), out[1] = mask mean.  dls = d(grad_scale*loss*n)/d l_s
// i.e. pass grad_scale = lambda_u / n for d(lambda_u * loss).  pl / mask_out / row_loss nullable.
int es_fm_consistency_fwd_bwd(const float* logits_w, int ldw, const float* logits_s, int lds, int n, int C,
                              float tau, float grad_scale, int* pseudo_label, uint8_t* mask, float* row_loss,
                              float* dlogits_s, int lddls, float* out, hipStream_t stream) {
  if (n <= 0 || C <= 0 || C > MAXC || ldw < C || lds < C || lddls < C) return ES_BAD_SHAPE;
  if (!logits_w || !logits_s || !dlogits_s || !out) return ES_BAD_ARG;
  hipLaunchKernelGGL(fm_consistency_kernel, 1, 256, 0, stream, logits_w, ldw, logits_s, lds, n, C, tau, grad_scale,
                     pseudo_label, mask, row_loss, dlogits_s, lddls, out);
  return hipGetLastError() == hipSuccess ? ES_OK : ES_HIP_ERROR;
}

// out[0] = poly loss (mean over n); dl = grad_scale * n * d(loss)/d l  (grad_scale = 1/n for d loss)
int es_poly_ce_fwd_bwd(const float* logits, int ldl, const int64_t* targets, const float* weights, int n, int C,
                       float epsilon, float grad_scale, float* dlogits, int lddl, float* out, hipStream_t stream) {
  if (n <= 0 || C <= 0 || C > MAXC || ldl < C || lddl < C) return ES_BAD_SHAPE;
  if (!logits || !targets || !dlogits || !out) return ES_BAD_ARG;
  hipLaunchKernelGGL(poly_ce_kernel, 1, 256, 0, stream, logits, ldl, targets, weights, n, C, epsilon, grad_scale,
                     dlogits, lddl, out);
  return hipGetLastError() == hipSuccess ? ES_OK : ES_HIP_ERROR;
}

// z [3 bs, L]: anchors, positives, negatives.  h_i = d_p,i - d_n,i + alpha; out = {mean max(h, 0), mean d_p,
// mean d_n, fraction of h > 0}; dz = grad_scale * d(sum_i max(h_i, 0))/dz, every row written (zeros for h <= 0)
int es_triplet_fwd_bwd(const float* z, int ldz, int bs, int L, float alpha, float grad_scale, float* dz, int lddz,
                       float* out, hipStream_t stream) {
  if (bs < 1 || bs > 0x7fffffff / 3 || L < 1 || L > 2048 || ldz < L || lddz < L) return ES_BAD_SHAPE;
  if (!z || !dz || !out) return ES_BAD_ARG;
  hipLaunchKernelGGL(triplet_kernel, 1, TRIPLET_THREADS, 0, stream, z, ldz, bs, L, alpha, grad_scale, dz, lddz, out);
  return hipGetLastError() == hipSuccess ? ES_OK : ES_HIP_ERROR;
}

// workspace of es_margin_softmax_fwd_bwd in floats: g [n, C], 1 / max(|x_i|, 1e-12) [n], row losses [n]
size_t es_margin_softmax_workspace(int n, int C) {
  if (n < 1 || C < 1 || C > MAXC) return 0;
  return (size_t)n * (size_t)(C + 2);
}

// AngularPenaltySMLoss.forward and its gradient (the header states the semantics).  Every check runs before the
// first launch; a refused call writes nothing.
int es_margin_softmax_fwd_bwd(const float* x, int ldx, const float* W, const float* bias, const int64_t* targets,
                              const float* class_weights, const float* mask, int n, int F, int C, int kind, float s,
                              float m, float eps, float grad_scale, float* dx, int lddx, float* dW, float* db,
                              float* out, float* row_loss, float* workspace, hipStream_t stream) {
  if (n < 1 || C < 1 || C > MAXC || F < 4 || F > MARGIN_MAXF || (F & 3) || ldx < F || lddx < F || (ldx & 3) ||
      (lddx & 3))
    return ES_BAD_ARG;
  if (kind < MARGIN_COSFACE || kind > MARGIN_ACLOSS || !(eps > 0.f && eps < 1.f)) return ES_BAD_ARG;
  if (!x || !W || !targets || !dx || !dW || !out || !workspace) return ES_BAD_ARG;
  if (((uintptr_t)x | (uintptr_t)W | (uintptr_t)dx | (uintptr_t)dW) & 15) return ES_BAD_ARG;
  if (((uintptr_t)workspace | (uintptr_t)out) & 3) return ES_BAD_ARG;
  const double k = 0.3, q = exp(-M_PI / 2.0 / k);  // g_theta's k (code/loss.py:262)
  MarginParams P;
  P.kind = kind;
  P.s = s;
  P.m = m;
  P.eps = eps;
  P.lo = (float)(-1.0 + (double)eps);
  P.hi = (float)(1.0 - (double)eps);
  P.cos_m = (float)cos((double)m);
  P.sin_m = (float)sin((double)m);
  P.sig1 = (float)((1.0 + q) / (1.0 - q));
  P.inv_k = (float)(1.0 / k);
  P.grad_scale = grad_scale;
  float* G = workspace;
  float* inv_norm = G + (size_t)n * C;
  float* ws_loss = inv_norm + n;
  hipLaunchKernelGGL(margin_rows_kernel, n, MARGIN_THREADS, 0, stream, x, ldx, W, bias, targets, class_weights, mask,
                     F, C, P, dx, lddx, G, inv_norm, ws_loss, row_loss);
  hipLaunchKernelGGL(margin_reduce_kernel, dim3((F / 4 + 63) / 64, C), 64, 0, stream, x, ldx, G, inv_norm, ws_loss, n,
                     F, C, grad_scale, dW, db, out);
  return hipGetLastError() == hipSuccess ? ES_OK : ES_HIP_ERROR;
}

// pred = argmax (first index on ties), conf = max softmax probability, label = conf > thres ? pred : 0;
// each output nullable, not all three
int es_softmax_predict(const float* logits, int ldl, int n, int C, float thres, int* pred, float* conf, int* label,
                       hipStream_t stream) {
  if (n <= 0 || C <= 0 || C > MAXC || ldl < C) return ES_BAD_SHAPE;
  if (!logits || (!pred && !conf && !label)) return ES_BAD_ARG;
  const int blocks = (n + 255) / 256 < 1024 ? (n + 255) / 256 : 1024;
  hipLaunchKernelGGL(softmax_predict_kernel, blocks, 256, 0, stream, logits, ldl, n, C, thres, pred, conf, label);
  return hipGetLastError() == hipSuccess ? ES_OK : ES_HIP_ERROR;
}

}  // extern "C"
