// DenseNet kernels (endossl/densenet.py: NativeDenseNet) for gfx950.
//
// A dense block lives in ONE NHWC buffer [rows, ld]: layer i reads the channel prefix [0, C_i) and writes its
// growth slice [C_i, C_i + 48) through the convs' element strides, so nothing is concatenated or copied.  The convs
// are conv.hip's / conv_bf16.hip's; what is specific to the layout is here, all bandwidth kernels (16-byte
// accesses along the channels, rows across the grid, fp32 arithmetic, fixed reduction orders):
//
//  es_conv2d_pack_bf16_pad(_multi)   fp32 [Cout][Cin][kh][kw] -> the two bf16 images at [Cout_p][Cin_p], zero rows /
//                                    columns in the padding (the bf16 convs take channel counts % 32; a prefix of
//                                    16 (mod 32) channels and the 48-channel slice are padded in the operands only)
//  es_dw_unpad_multi                 padded weight gradients -> the true [Cout][Cin][kh kw] tensors
//  es_bn2d_stats_ld_ex               mean / rstd / centred square sum of a row-strided [rows, C] view
//  es_bn2d_stats_from_partials       the same from a conv epilogue's bn_partials, at an offset of the block arrays
//  es_bn2d_running_multi             the train-mode running-buffer update of every BatchNorm over one statistics array
//  es_bn2d_eval_stats                running buffers -> mean / rstd arrays (zero-padded) for the eval-mode gathers
//  es_bn2d_apply_ld_ex               y = (relu) bn(x) between row-strided views
//  es_bn2d_bwd_recompute_ld_ex       es_bn2d_bwd_recompute_ex with row strides, fp32 / accumulating dx
//  es_avgpool2_ld_fwd_ex / _bwd_ex   2 x 2 / 2 average pool into / out of a row-strided view
//
// The BatchNorm kernels reduce through bn_rows.h, the code conv.hip's dense kernels run: on a contiguous input they
// give the same bits.
#include "common.h"
#include "bn_rows.h"

namespace {

inline bool dn_al16(const void* p) { return ((uintptr_t)p & 15) == 0; }
inline int dn_grid(long n) {
  long b = (n + 255) / 256;
  return (int)(b > 16384 ? 16384 : (b < 1 ? 1 : b));
}

// ---- padded weight images ---------------------------------------------------------------------------------
struct PadPackEntry {
  const float* w;
  bf16 *wp, *wt;
  int Cout, Cin, T, Cout_p, Cin_p, pad;
};
// wp[co][tap][ci] over [Cout_p][T][Cin_p], wt[ci][tap][co] over [Cin_p][T][Cout_p]; 8 consecutive elements of the
// inner dimension per thread (one 16-byte store; Cout_p, Cin_p % 8 == 0), zero outside [Cout) x [Cin).
__global__ __launch_bounds__(256) void pack_pad_kernel(const PadPackEntry* __restrict__ tab, PadPackEntry one) {
  const PadPackEntry e = tab ? tab[blockIdx.y] : one;
  const long np = (long)e.Cout_p * e.T * (e.Cin_p / 8);
  const bf16 z = (bf16)0.f;
  if (e.wp) {
    const int c8n = e.Cin_p / 8;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < np; i += (long)gridDim.x * blockDim.x) {
      const int ci0 = (int)(i % c8n) * 8;
      const long t2 = i / c8n;
      const int tap = (int)(t2 % e.T), co = (int)(t2 / e.T);
      bf16x8 v;
#pragma unroll
      for (int j = 0; j < 8; ++j)
        v[j] = (co < e.Cout && ci0 + j < e.Cin) ? (bf16)e.w[((long)co * e.Cin + ci0 + j) * e.T + tap] : z;
      *(bf16x8*)(e.wp + i * 8) = v;
    }
  }
  if (e.wt) {
    const int c8n = e.Cout_p / 8;
    const long nt = (long)e.Cin_p * e.T * c8n;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < nt; i += (long)gridDim.x * blockDim.x) {
      const int co0 = (int)(i % c8n) * 8;
      const long t2 = i / c8n;
      const int tap = (int)(t2 % e.T), ci = (int)(t2 / e.T);
      bf16x8 v;
#pragma unroll
      for (int j = 0; j < 8; ++j)
        v[j] = (ci < e.Cin && co0 + j < e.Cout) ? (bf16)e.w[((long)(co0 + j) * e.Cin + ci) * e.T + tap] : z;
      *(bf16x8*)(e.wt + i * 8) = v;
    }
  }
}

inline bool pad_entry_ok(const PadPackEntry& e) {
  return e.w && (e.wp || e.wt) && e.Cout > 0 && e.Cin > 0 && e.T > 0 && e.Cout_p >= e.Cout && e.Cin_p >= e.Cin &&
         e.Cout_p % 8 == 0 && e.Cin_p % 8 == 0 && (!e.wp || dn_al16(e.wp)) && (!e.wt || dn_al16(e.wt));
}

// dst[co][ci][tap] = src[co][ci][tap] of a [Cout_p][Cin_p][T] gradient: row co's first Cin T floats are the true
// row, so each row is one contiguous copy (float4 where Cin T % 4 == 0 and both pointers are 16-byte aligned)
struct UnpadEntry {
  const float* src;
  float* dst;
  int Cout_p, Cin_p, Cout, Cin, T, pad;
};
__global__ __launch_bounds__(256) void dw_unpad_kernel(const UnpadEntry* __restrict__ tab) {
  const UnpadEntry e = tab[blockIdx.y];
  const int rowlen = e.Cin * e.T;
  const long srow = (long)e.Cin_p * e.T;
  if (rowlen % 4 == 0 && srow % 4 == 0 && (((uintptr_t)e.src | (uintptr_t)e.dst) & 15) == 0) {
    const int r4 = rowlen / 4;
    const long n = (long)e.Cout * r4;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
      const int co = (int)(i / r4), q = (int)(i % r4);
      *(f32x4*)(e.dst + (long)co * rowlen + 4 * q) = *(const f32x4*)(e.src + co * srow + 4 * q);
    }
  } else {
    const long n = (long)e.Cout * rowlen;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
      const int co = (int)(i / rowlen), q = (int)(i % rowlen);
      e.dst[i] = e.src[co * srow + q];
    }
  }
}

// ---- shared batch statistics ------------------------------------------------------------------------------
// rstd from the centred square sum, chan_final_kernel<2>'s expression
__global__ void stats_m2_kernel(const float* __restrict__ m2, int C, int rows, float eps, float* __restrict__ rstd) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const float var = m2[c] / (float)rows;
  rstd[c] = 1.0f / sqrtf(var + eps);
}

struct RunEntry {
  float *rm, *rv;
  int64_t* nbt;
  int C, off;
};
// running <- (1 - m) running + m (mean, M2 / (rows - 1)), num_batches_tracked += 1: the expressions of
// chan_final_kernel<2> / bn_stats_from_partials_kernel, for entry blockIdx.y over stats[off .. off + C)
__global__ __launch_bounds__(256) void running_multi_kernel(const RunEntry* __restrict__ tab,
                                                            const float* __restrict__ mean,
                                                            const float* __restrict__ m2, int rows, float momentum) {
  const RunEntry e = tab[blockIdx.y];
  if (blockIdx.x == 0 && threadIdx.x == 0 && e.nbt) *e.nbt += 1;
  for (int c = blockIdx.x * blockDim.x + threadIdx.x; c < e.C; c += gridDim.x * blockDim.x) {
    const float mu = mean[e.off + c], M2 = m2[e.off + c];
    const float var = M2 / (float)rows;
    const float unb = rows > 1 ? M2 / (float)(rows - 1) : var;
    e.rm[c] = (1.f - momentum) * e.rm[c] + momentum * mu;
    e.rv[c] = (1.f - momentum) * e.rv[c] + momentum * unb;
  }
}

// eval mode: mean = running_mean, rstd = 1 / sqrt(running_var + eps) (bn_eval_rstd: the bits every eval-mode
// apply kernel uses), zeros over [C, Cp)
__global__ void eval_stats_kernel(const float* __restrict__ rm, const float* __restrict__ rv, int C, int Cp, float eps,
                                  float* __restrict__ mean, float* __restrict__ rstd) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= Cp) return;
  mean[c] = c < C ? rm[c] : 0.f;
  rstd[c] = c < C ? bn_eval_rstd(rv[c], eps) : 0.f;
}

// ---- BatchNorm apply / backward between row-strided views ----------------------------------------------------
// y[r][c] = (relu) bn_affine(x[r][c]) for c < C: bn_apply_kernel's arithmetic and rounding
template <int VEC, typename TI, typename TO>
__global__ void bn_apply_ld_kernel(const TI* __restrict__ x, long ldx, int rows, int CV,
                                   const float* __restrict__ mean, const float* __restrict__ rstd,
                                   const float* __restrict__ gamma, const float* __restrict__ beta, int relu,
                                   TO* __restrict__ y, long ldy) {
  const long nv = (long)rows * CV;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += (long)gridDim.x * blockDim.x) {
    const long r = i / CV;
    const int c = (int)(i - r * CV) * VEC;
    float xv[VEC], mu[VEC], rs[VEC], ga[VEC], be[VEC], o[VEC];
    ldv<VEC>(x + r * ldx + c, xv);
    ldv<VEC>(mean + c, mu);
    ldv<VEC>(rstd + c, rs);
    ldv<VEC>(gamma + c, ga);
    ldv<VEC>(beta + c, be);
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      o[j] = bn_affine(xv[j], mu[j], rs[j], ga[j], be[j]);
      if (relu) o[j] = fmaxf(o[j], 0.f);
    }
    stv<VEC>(y + r * ldy + c, o);
  }
}

// dx[r][c] (+)= bn_bwd_dx(...) with the ReLU mask rebuilt from x (bn_bwd_apply_kernel<VEC, T, true>'s arithmetic);
// TD = dx's element type, an accumulating store adds in fp32
template <int VEC, typename T, typename TD>
__global__ void bn_bwd_apply_ld_kernel(const T* __restrict__ x, long ldx, const T* __restrict__ dy, long ldy, int rows,
                                       int CV, const float* __restrict__ mean, const float* __restrict__ rstd,
                                       const float* __restrict__ gamma, const float* __restrict__ beta,
                                       const float* __restrict__ sums, TD* __restrict__ dx, long lddx, int accumulate) {
  const float inv = 1.0f / (float)rows;
  const int C = CV * VEC;
  const long nv = (long)rows * CV;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += (long)gridDim.x * blockDim.x) {
    const long r = i / CV;
    const int c = (int)(i - r * CV) * VEC;
    float xv[VEC], gg[VEC], mu[VEC], rs[VEC], ga[VEC], be[VEC], s0[VEC], s1[VEC], o[VEC];
    ldv<VEC>(x + r * ldx + c, xv);
    ldv<VEC>(dy + r * ldy + c, gg);
    ldv<VEC>(mean + c, mu);
    ldv<VEC>(rstd + c, rs);
    ldv<VEC>(gamma + c, ga);
    ldv<VEC>(beta + c, be);
    ldv<VEC>(sums + c, s0);
    ldv<VEC>(sums + C + c, s1);
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      if (!bn_relu_live<T>(xv[j], mu[j], rs[j], ga[j], be[j])) gg[j] = 0.f;
      o[j] = bn_bwd_dx(xv[j], gg[j], mu[j], rs[j], ga[j], s0[j], s1[j], inv);
    }
    if (accumulate) {
      float p[VEC];
      ldv<VEC>(dx + r * lddx + c, p);
#pragma unroll
      for (int j = 0; j < VEC; ++j) o[j] = p[j] + o[j];
    }
    stv<VEC>(dx + r * lddx + c, o);
  }
}

template <typename T, typename TD>
void bwd_ld_launch(bool v4, const T* x, long ldx, const T* dy, long ldy, int rows, int C, const float* mean,
                   const float* rstd, const float* gamma, const float* beta, const float* sums, TD* dx, long lddx,
                   int accumulate, hipStream_t stream) {
  if (v4)
    hipLaunchKernelGGL((bn_bwd_apply_ld_kernel<4, T, TD>), dn_grid((long)rows * (C / 4)), 256, 0, stream, x, ldx, dy, ldy,
                       rows, C / 4, mean, rstd, gamma, beta, sums, dx, lddx, accumulate);
  else
    hipLaunchKernelGGL((bn_bwd_apply_ld_kernel<1, T, TD>), dn_grid((long)rows * C), 256, 0, stream, x, ldx, dy, ldy,
                       rows, C, mean, rstd, gamma, beta, sums, dx, lddx, accumulate);
}

template <typename T>
int bwd_recompute_ld_impl(const T* x, long ldx, const T* dy, long ldy, int rows, int C, const float* gamma,
                          const float* beta, const float* mean, const float* rstd, void* dx, long lddx, int dx_fp32,
                          int dx_accumulate, float* dgamma, float* dbeta, int accumulate, float* workspace,
                          hipStream_t stream) {
  const int G = chan_groups(rows);
  const int per = (rows + G - 1) / G;
  float* sums = workspace + (size_t)G * 2 * C;
  const bool v4 = C % 4 == 0 && ldx % 4 == 0 && ldy % 4 == 0 && lddx % 4 == 0 && dn_al16(x) && dn_al16(dy) &&
                  dn_al16(dx) && dn_al16(mean) && dn_al16(rstd) && dn_al16(gamma) && dn_al16(beta) && dn_al16(sums);
  // the dense backward's partial sums (chan_partial_kernel<2, ., T, true>) over x's rows at ldx and dy's at ldy
  const RowMap rm{(long)rows * ldx, ldx, rows};
  if (v4)
    hipLaunchKernelGGL((chan_partial_kernel<2, 4, T, true>), G, 256, 0, stream, x, rm, rows, C, per, mean, rstd, dy,
                       (const T*)nullptr, 1, workspace, gamma, beta, ldy);
  else
    hipLaunchKernelGGL((chan_partial_kernel<2, 1, T, true>), G, 256, 0, stream, x, rm, rows, C, per, mean, rstd, dy,
                       (const T*)nullptr, 1, workspace, gamma, beta, ldy);
  ChanFin f{dbeta, dgamma, sums, nullptr, nullptr, nullptr, 0.f, 0.f, rows, C, accumulate};
  hipLaunchKernelGGL(chan_final_kernel<3>, (2 * C + 15) / 16, 256, 0, stream, workspace, G, 2 * C, f);
  if (dx_fp32)
    bwd_ld_launch<T, float>(v4, x, ldx, dy, ldy, rows, C, mean, rstd, gamma, beta, sums, (float*)dx, lddx,
                            dx_accumulate, stream);
  else
    bwd_ld_launch<T, T>(v4, x, ldx, dy, ldy, rows, C, mean, rstd, gamma, beta, sums, (T*)dx, lddx, dx_accumulate,
                        stream);
  return hipGetLastError() == hipSuccess ? ES_OK : ES_HIP_ERROR;
}

template <typename T>
int stats_ld_impl(const T* x, int rows, int C, long ld, float eps, float* mean, float* rstd, float* m2,
                  float* workspace, hipStream_t stream) {
  const int G = chan_groups(rows);
  const int per = (rows + G - 1) / G;
  const RowMap rm{(long)rows * ld, ld, rows};  // contiguous in chan_partial_kernel's sense: row r at r * ld
  const bool v4 = C % 4 == 0 && ld % 4 == 0 && dn_al16(x) && dn_al16(mean);
  const dim3 fg((C + 15) / 16);
  ChanFin fm{mean, nullptr, nullptr, nullptr, nullptr, nullptr, 0.f, 0.f, rows, 0, 0};
  ChanFin f2{m2, nullptr, nullptr, nullptr, nullptr, nullptr, 0.f, 0.f, rows, 0, 0};
  if (v4)
    hipLaunchKernelGGL((chan_partial_kernel<0, 4, T>), G, 256, 0, stream, x, rm, rows, C, per, nullptr, nullptr, nullptr,
                       nullptr, 0, workspace, nullptr, nullptr);
  else
    hipLaunchKernelGGL((chan_partial_kernel<0, 1, T>), G, 256, 0, stream, x, rm, rows, C, per, nullptr, nullptr, nullptr,
                       nullptr, 0, workspace, nullptr, nullptr);
  hipLaunchKernelGGL(chan_final_kernel<1>, fg, 256, 0, stream, workspace, G, C, fm);
  if (v4)
    hipLaunchKernelGGL((chan_partial_kernel<1, 4, T>), G, 256, 0, stream, x, rm, rows, C, per, mean, nullptr, nullptr,
                       nullptr, 0, workspace, nullptr, nullptr);
  else
    hipLaunchKernelGGL((chan_partial_kernel<1, 1, T>), G, 256, 0, stream, x, rm, rows, C, per, mean, nullptr, nullptr,
                       nullptr, 0, workspace, nullptr, nullptr);
  hipLaunchKernelGGL(chan_final_kernel<0>, fg, 256, 0, stream, workspace, G, C, f2);
  hipLaunchKernelGGL(stats_m2_kernel, (C + 255) / 256, 256, 0, stream, m2, C, rows, eps, rstd);
  return hipGetLastError() == hipSuccess ? ES_OK : ES_HIP_ERROR;
}

// ---- 2 x 2 / 2 average pool, one side row-strided (avgpool_fwd_kernel's sum order: (0 + a + b + c + d) / 4) ----
template <int VEC, typename TI, typename TO>
__global__ void avgpool2_ld_fwd_kernel(const TI* __restrict__ x, int N, int H, int W, int CV, int Ho, int Wo,
                                       TO* __restrict__ y, long ldy) {
  const long n_out = (long)N * Ho * Wo * CV;
  const int C = CV * VEC;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n_out; i += (long)gridDim.x * blockDim.x) {
    const int c = (int)(i % CV) * VEC;
    const long pix = i / CV;  // (n Ho + ho) Wo + wo
    const int wo = (int)(pix % Wo);
    const long t = pix / Wo;
    const int ho = (int)(t % Ho), n = (int)(t / Ho);
    float s[VEC], a[VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) s[j] = 0.f;
#pragma unroll
    for (int ky = 0; ky < 2; ++ky)
#pragma unroll
      for (int kx = 0; kx < 2; ++kx) {
        ldv<VEC>(x + (((long)n * H + 2 * ho + ky) * W + 2 * wo + kx) * C + c, a);
#pragma unroll
        for (int j = 0; j < VEC; ++j) s[j] += a[j];
      }
#pragma unroll
    for (int j = 0; j < VEC; ++j) s[j] *= 0.25f;
    stv<VEC>(y + pix * ldy + c, s);
  }
}
// dx[n][h][w][c] = dy[n][h / 2][w / 2][c] / 4 (0 past the pooled extent of an odd map); dy row-strided
template <int VEC, typename TI, typename TO>
__global__ void avgpool2_ld_bwd_kernel(const TI* __restrict__ dy, long lddy, int N, int H, int W, int CV, int Ho,
                                       int Wo, TO* __restrict__ dx) {
  const long n_in = (long)N * H * W * CV;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n_in; i += (long)gridDim.x * blockDim.x) {
    const int c = (int)(i % CV) * VEC;
    const long pix = i / CV;
    const int w = (int)(pix % W);
    const long t = pix / W;
    const int h = (int)(t % H), n = (int)(t / H);
    float v[VEC];
    if (h / 2 < Ho && w / 2 < Wo) {
      ldv<VEC>(dy + (((long)n * Ho + h / 2) * Wo + w / 2) * lddy + c, v);
#pragma unroll
      for (int j = 0; j < VEC; ++j) v[j] *= 0.25f;
    } else {
#pragma unroll
      for (int j = 0; j < VEC; ++j) v[j] = 0.f;
    }
    stv<VEC>(dx + pix * (long)(CV * VEC) + c, v);
  }
}

template <typename TI, typename TO>
void pool_fwd_launch(const void* x, int N, int H, int W, int C, void* y, long ldy, hipStream_t stream) {
  const int Ho = H / 2, Wo = W / 2;
  const bool v4 = C % 4 == 0 && ldy % 4 == 0 && dn_al16(x) && dn_al16(y);
  if (v4)
    hipLaunchKernelGGL((avgpool2_ld_fwd_kernel<4, TI, TO>), dn_grid((long)N * Ho * Wo * (C / 4)), 256, 0, stream,
                       (const TI*)x, N, H, W, C / 4, Ho, Wo, (TO*)y, ldy);
  else
    hipLaunchKernelGGL((avgpool2_ld_fwd_kernel<1, TI, TO>), dn_grid((long)N * Ho * Wo * C), 256, 0, stream,
                       (const TI*)x, N, H, W, C, Ho, Wo, (TO*)y, ldy);
}
template <typename TI, typename TO>
void pool_bwd_launch(const void* dy, long lddy, int N, int H, int W, int C, void* dx, hipStream_t stream) {
  const int Ho = H / 2, Wo = W / 2;
  const bool v4 = C % 4 == 0 && lddy % 4 == 0 && dn_al16(dy) && dn_al16(dx);
  if (v4)
    hipLaunchKernelGGL((avgpool2_ld_bwd_kernel<4, TI, TO>), dn_grid((long)N * H * W * (C / 4)), 256, 0, stream,
                       (const TI*)dy, lddy, N, H, W, C / 4, Ho, Wo, (TO*)dx);
  else
    hipLaunchKernelGGL((avgpool2_ld_bwd_kernel<1, TI, TO>), dn_grid((long)N * H * W * C), 256, 0, stream,
                       (const TI*)dy, lddy, N, H, W, C, Ho, Wo, (TO*)dx);
}

}  // namespace

extern "C" {

// fp32 w [Cout][Cin][kh][kw] -> wp [Cout_p][kh kw][Cin_p] and wt [Cin_p][kh kw][Cout_p] (bf16, either nullable),
// es_conv2d_pack_bf16's element mapping and rounding with zeros in the padding.  Cout_p, Cin_p % 8 == 0.
int es_conv2d_pack_bf16_pad(const float* w, int Cout, int Cin, int kh, int kw, int Cout_p, int Cin_p, void* wp, void* wt,
                            hipStream_t stream) {
  if (kh <= 0 || kw <= 0) return ES_BAD_SHAPE;
  const PadPackEntry e{w, (bf16*)wp, (bf16*)wt, Cout, Cin, kh * kw, Cout_p, Cin_p, 0};
  if (!w || (!wp && !wt)) return ES_BAD_ARG;
  if (!pad_entry_ok(e)) return ES_BAD_SHAPE;
  const long b = ((long)Cout_p * Cin_p * e.T / 8 + 255) / 256;
  hipLaunchKernelGGL(pack_pad_kernel, dim3((unsigned)(b > 1024 ? 1024 : b), 1), 256, 0, stream, nullptr, e);
  return hipGetLastError() == hipSuccess ? ES_OK : ES_HIP_ERROR;
}

int es_conv_pack_pad_entry_size(void) { return (int)sizeof(PadPackEntry); }

// es_conv2d_pack_bf16_pad over n weights in one launch: table = n device-resident entries of
// es_conv_pack_pad_entry_size() bytes {const float* w; void* wp; void* wt; int Cout, Cin, kh_x_kw, Cout_p, Cin_p, 0};
// max_elems = the largest Cout_p * Cin_p * kh * kw (sizes the grid).  The caller has checked each entry as
// es_conv2d_pack_bf16_pad does.
int es_conv2d_pack_bf16_pad_multi(const void* table, int n, long max_elems, hipStream_t stream) {
  if (!table) return ES_BAD_ARG;
  if (n <= 0 || max_elems <= 0) return ES_BAD_SHAPE;
  const long b = (max_elems / 8 + 255) / 256;
  hipLaunchKernelGGL(pack_pad_kernel, dim3((unsigned)(b > 1024 ? 1024 : (b < 1 ? 1 : b)), n), 256, 0, stream,
                     (const PadPackEntry*)table, PadPackEntry{});
  return hipGetLastError() == hipSuccess ? ES_OK : ES_HIP_ERROR;
}

int es_dw_unpad_entry_size(void) { return (int)sizeof(UnpadEntry); }

// table = n device-resident entries of es_dw_unpad_entry_size() bytes {const float* src; float* dst; int Cout_p,
// Cin_p, Cout, Cin, kh_x_kw, 0}: dst [Cout][Cin][kh kw] = the true rows / columns of src [Cout_p][Cin_p][kh kw]
// (overwritten).  max_elems = the largest Cout * Cin * kh * kw.
int es_dw_unpad_multi(const void* table, int n, long max_elems, hipStream_t stream) {
  if (!table) return ES_BAD_ARG;
  if (n <= 0 || max_elems <= 0) return ES_BAD_SHAPE;
  const long b = (max_elems / 4 + 255) / 256;
  hipLaunchKernelGGL(dw_unpad_kernel, dim3((unsigned)(b > 1024 ? 1024 : (b < 1 ? 1 : b)), n), 256, 0, stream,
                     (const UnpadEntry*)table);
  return hipGetLastError() == hipSuccess ? ES_OK : ES_HIP_ERROR;
}

// Batch statistics of the row-strided view x[r * ld + c], r < rows, c < C: mean, rstd = 1 / sqrt(var + eps) (biased
// variance) and m2 = the centred square sum (what the running update needs).  The sums of es_bn2d_fwd_ex's
// statistics passes: the same mean / rstd on a contiguous copy.  workspace: es_chan_workspace(rows, C) floats.
// flags bit 0: x is bf16.
int es_bn2d_stats_ld_ex(const void* x, int rows, int C, long ld, float eps, float* mean, float* rstd, float* m2,
                        float* workspace, int flags, hipStream_t stream) {
  if (!x || !mean || !rstd || !m2 || !workspace) return ES_BAD_ARG;
  if (rows <= 0 || C <= 0 || ld < C || (flags & ~1) || (long)rows * ld >= (1L << 31)) return ES_BAD_SHAPE;
  return (flags & 1) ? stats_ld_impl<bf16>((const bf16*)x, rows, C, ld, eps, mean, rstd, m2, workspace, stream)
                     : stats_ld_impl<float>((const float*)x, rows, C, ld, eps, mean, rstd, m2, workspace, stream);
}

// The same three arrays from a bf16 conv's bn_partials (es_conv2d_bnstats_size(rows, PC) floats, PC = the conv's
// (padded) output channels, the first C of them taken): es_bn2d_fwd_partials_ex's combination, bit for bit, without
// the running-buffer update.  The partials are overwritten (as there).
int es_bn2d_stats_from_partials(float* partials, int rows, int C, int PC, float eps, float* mean, float* rstd, float* m2,
                                hipStream_t stream) {
  if (!partials || !mean || !rstd || !m2) return ES_BAD_ARG;
  if (rows <= 0 || C <= 0 || PC < C) return ES_BAD_SHAPE;
  const int nblk = (rows + 127) / 128, G = 64;
  if (nblk > G) {
    const int ng = (nblk + G - 1) / G;
    hipLaunchKernelGGL(bn_stats_from_partials_kernel<false>, dim3((C + 63) / 64, ng), 256, 0, stream, partials, nblk, 128,
                       1, G, rows, C, PC, eps, 0.f, mean, rstd, nullptr, nullptr, nullptr, nullptr);
    hipLaunchKernelGGL(bn_stats_from_partials_kernel<true>, dim3((C + 63) / 64, 1), 256, 0, stream, partials, ng,
                       128 * G, G, ng, rows, C, PC, eps, 0.f, mean, rstd, nullptr, nullptr, nullptr, m2);
  } else {
    hipLaunchKernelGGL(bn_stats_from_partials_kernel<true>, dim3((C + 63) / 64, 1), 256, 0, stream, partials, nblk, 128,
                       1, nblk, rows, C, PC, eps, 0.f, mean, rstd, nullptr, nullptr, nullptr, m2);
  }
  return hipGetLastError() == hipSuccess ? ES_OK : ES_HIP_ERROR;
}

int es_bn_running_entry_size(void) { return (int)sizeof(RunEntry); }

// Train-mode running-buffer update of n BatchNorms that share one statistics array: table = n device-resident
// entries of es_bn_running_entry_size() bytes {float* running_mean; float* running_var; int64* num_batches_tracked;
// int C; int offset}; entry j takes mean / m2 [offset, offset + C).  momentum blend with the unbiased variance
// m2 / (rows - 1), num_batches_tracked += 1 -- es_bn2d_fwd_ex's / es_bn2d_fwd_partials_ex's update.
int es_bn2d_running_multi(const void* table, int n, int max_c, const float* mean, const float* m2, int rows,
                          float momentum, hipStream_t stream) {
  if (!table || !mean || !m2) return ES_BAD_ARG;
  if (n <= 0 || max_c <= 0 || rows <= 0) return ES_BAD_SHAPE;
  hipLaunchKernelGGL(running_multi_kernel, dim3((max_c + 255) / 256, n), 256, 0, stream, (const RunEntry*)table, mean,
                     m2, rows, momentum);
  return hipGetLastError() == hipSuccess ? ES_OK : ES_HIP_ERROR;
}

// mean[c] = running_mean[c], rstd[c] = 1 / sqrt(running_var[c] + eps) for c < C, zeros over [C, Cp)
int es_bn2d_eval_stats(const float* running_mean, const float* running_var, int C, int Cp, float eps, float* mean,
                       float* rstd, hipStream_t stream) {
  if (!running_mean || !running_var || !mean || !rstd) return ES_BAD_ARG;
  if (C <= 0 || Cp < C) return ES_BAD_SHAPE;
  hipLaunchKernelGGL(eval_stats_kernel, (Cp + 255) / 256, 256, 0, stream, running_mean, running_var, C, Cp, eps, mean,
                     rstd);
  return hipGetLastError() == hipSuccess ? ES_OK : ES_HIP_ERROR;
}

// y[r * ldy + c] = bn(x[r * ldx + c]) (then ReLU if relu) with the given mean / rstd, es_bn2d_fwd_ex's affine map and
// rounding.  flags bit 0: x is bf16, bit 1: y is bf16.
int es_bn2d_apply_ld_ex(const void* x, long ldx, int rows, int C, const float* mean, const float* rstd,
                        const float* gamma, const float* beta, int relu, void* y, long ldy, int flags,
                        hipStream_t stream) {
  if (!x || !y || !mean || !rstd || !gamma || !beta) return ES_BAD_ARG;
  if (rows <= 0 || C <= 0 || ldx < C || ldy < C || (flags & ~3)) return ES_BAD_SHAPE;
  const bool v4 = C % 4 == 0 && ldx % 4 == 0 && ldy % 4 == 0 && dn_al16(x) && dn_al16(y) && dn_al16(mean) &&
                  dn_al16(rstd) && dn_al16(gamma) && dn_al16(beta);
#define ES_DN_APPLY(TI, TO)                                                                                             \
  do {                                                                                                                  \
    if (v4)                                                                                                             \
      hipLaunchKernelGGL((bn_apply_ld_kernel<4, TI, TO>), dn_grid((long)rows * (C / 4)), 256, 0, stream, (const TI*)x,  \
                         ldx, rows, C / 4, mean, rstd, gamma, beta, relu, (TO*)y, ldy);                                 \
    else                                                                                                                \
      hipLaunchKernelGGL((bn_apply_ld_kernel<1, TI, TO>), dn_grid((long)rows * C), 256, 0, stream, (const TI*)x, ldx,   \
                         rows, C, mean, rstd, gamma, beta, relu, (TO*)y, ldy);                                          \
  } while (0)
  if (flags == 3) ES_DN_APPLY(bf16, bf16);
  else if (flags == 1) ES_DN_APPLY(bf16, float);
  else if (flags == 2) ES_DN_APPLY(float, bf16);
  else ES_DN_APPLY(float, float);
#undef ES_DN_APPLY
  return hipGetLastError() == hipSuccess ? ES_OK : ES_HIP_ERROR;
}

// es_bn2d_bwd_recompute_ex between row-strided views: x[r * ldx + c], dy[r * ldy + c], dx[r * lddx + c], c < C.
// flags bit 0: x and dy are bf16 maps; bit 1: dx is fp32 whatever the maps are (else the maps' type); bit 2: dx
// accumulates (added in fp32).  dgamma / dbeta (+)= as the dense entry point (`accumulate`).  Columns >= C of every
// view are neither read nor written.  workspace: es_chan_workspace(rows, C) floats.  Same reduction order as
// es_bn2d_bwd_recompute_ex: on contiguous views the same dx / dgamma / dbeta bits.
int es_bn2d_bwd_recompute_ld_ex(const void* x, long ldx, const void* dy, long ldy, int rows, int C, const float* gamma,
                                const float* beta, const float* mean, const float* rstd, void* dx, long lddx,
                                float* dgamma, float* dbeta, int accumulate, float* workspace, int flags,
                                hipStream_t stream) {
  if (!x || !dy || !dx || !gamma || !beta || !mean || !rstd || !dgamma || !dbeta || !workspace) return ES_BAD_ARG;
  if (rows <= 0 || C <= 0 || ldx < C || ldy < C || lddx < C || (flags & ~7)) return ES_BAD_SHAPE;
  if ((long)rows * ldx >= (1L << 31) || (long)rows * ldy >= (1L << 31) || (long)rows * lddx >= (1L << 31))
    return ES_BAD_SHAPE;
  const int f32dx = (flags & 2) || !(flags & 1), acc = (flags >> 2) & 1;
  if (flags & 1)
    return bwd_recompute_ld_impl<bf16>((const bf16*)x, ldx, (const bf16*)dy, ldy, rows, C, gamma, beta, mean, rstd, dx,
                                       lddx, f32dx, acc, dgamma, dbeta, accumulate, workspace, stream);
  return bwd_recompute_ld_impl<float>((const float*)x, ldx, (const float*)dy, ldy, rows, C, gamma, beta, mean, rstd, dx,
                                      lddx, 1, acc, dgamma, dbeta, accumulate, workspace, stream);
}

// AvgPool2d(2, 2) of the dense NHWC map x [N, H, W, C] into the row-strided view y[((n Ho + ho) Wo + wo) * ldy + c]
// (Ho = H / 2, Wo = W / 2): es_avgpool2d_fwd_ex's values.  flags bit 0: x is bf16, bit 1: y is bf16.
int es_avgpool2_ld_fwd_ex(const void* x, int N, int H, int W, int C, void* y, long ldy, int flags, hipStream_t stream) {
  if (!x || !y) return ES_BAD_ARG;
  if (N <= 0 || H < 2 || W < 2 || C <= 0 || ldy < C || (flags & ~3)) return ES_BAD_SHAPE;
  if (flags == 3) pool_fwd_launch<bf16, bf16>(x, N, H, W, C, y, ldy, stream);
  else if (flags == 1) pool_fwd_launch<bf16, float>(x, N, H, W, C, y, ldy, stream);
  else if (flags == 2) pool_fwd_launch<float, bf16>(x, N, H, W, C, y, ldy, stream);
  else pool_fwd_launch<float, float>(x, N, H, W, C, y, ldy, stream);
  return hipGetLastError() == hipSuccess ? ES_OK : ES_HIP_ERROR;
}

// Its backward: dx [N, H, W, C] dense (overwritten) = dy[((n Ho + h / 2) Wo + w / 2) * lddy + c] / 4.
// flags bit 0: dy is bf16, bit 1: dx is bf16.
int es_avgpool2_ld_bwd_ex(const void* dy, long lddy, int N, int H, int W, int C, void* dx, int flags,
                          hipStream_t stream) {
  if (!dy || !dx) return ES_BAD_ARG;
  if (N <= 0 || H < 2 || W < 2 || C <= 0 || lddy < C || (flags & ~3)) return ES_BAD_SHAPE;
  if (flags == 3) pool_bwd_launch<bf16, bf16>(dy, lddy, N, H, W, C, dx, stream);
  else if (flags == 1) pool_bwd_launch<bf16, float>(dy, lddy, N, H, W, C, dx, stream);
  else if (flags == 2) pool_bwd_launch<float, bf16>(dy, lddy, N, H, W, C, dx, stream);
  else pool_bwd_launch<float, float>(dy, lddy, N, H, W, C, dx, stream);
  return hipGetLastError() == hipSuccess ? ES_OK : ES_HIP_ERROR;
}

}  // extern "C"
