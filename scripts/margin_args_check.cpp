// Host-only check of es_margin_softmax_fwd_bwd's argument validation: every call below must be refused with
// -2 (bad argument) before any launch, so the program needs no GPU and the pointers are never followed.
// Built against csrc/losses.hip itself with the host side under AddressSanitizer + UBSan:
//
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined \
//       -I endoscopy-image-classification_amd/csrc -I include \
//       scripts/margin_args_check.cpp endoscopy-image-classification_amd/csrc/losses.hip -o margin_args_check
//   ./margin_args_check
#include <cstdint>
#include <cstdio>
#include <vector>

#include "endossl.h"

namespace {

struct Args {
  const float* x;
  int ldx;
  const float* W;
  const float* bias;
  const int64_t* y;
  const float* cw;
  const float* mask;
  int n, F, C, kind;
  float* dx;
  int lddx;
  float* dW;
  float* db;
  float* out;
  float* row_loss;
  float* ws;
};

int run(const Args& a) {
  return es_margin_softmax_fwd_bwd(a.x, a.ldx, a.W, a.bias, a.y, a.cw, a.mask, a.n, a.F, a.C, a.kind, 30.f, 0.3f, 1e-7f,
                                   1.f / 8, a.dx, a.lddx, a.dW, a.db, a.out, a.row_loss, a.ws, nullptr);
}

int failures = 0;

void expect_refused(const char* what, const Args& a) {
  const int rc = run(a);
  if (rc != -2) {
    std::printf("FAIL %-28s returned %d, expected -2\n", what, rc);
    ++failures;
  } else {
    std::printf("ok   %-28s -> -2\n", what);
  }
}

}  // namespace

int main() {
  // host buffers of the right sizes, 16-byte aligned: validation must return before touching them
  const int n = 8, F = 64, C = 23;
  std::vector<float> store(4 + n * F * 2 + C * F * 2 + n * (C + 2) + 64, 0.f);
  float* base = store.data();
  while (reinterpret_cast<uintptr_t>(base) & 15) ++base;
  float* x = base;
  float* W = x + n * F;
  float* dx = W + C * F;
  float* dW = dx + n * F;
  float* ws = dW + C * F;
  float* out = ws + n * (C + 2);
  std::vector<int64_t> y(n, 0);
  const Args good{x, F, W, nullptr, y.data(), nullptr, nullptr, n, F, C, 1, dx, F, dW, nullptr, out, nullptr, ws};

  Args a = good;
  a.C = 65;
  expect_refused("C = 65", a);
  a = good;
  a.C = 0;
  expect_refused("C = 0", a);
  a = good;
  a.F = 6;
  expect_refused("F = 6", a);
  a = good;
  a.F = 2052;
  a.ldx = a.lddx = 2052;
  expect_refused("F = 2052", a);
  a = good;
  a.F = 0;
  expect_refused("F = 0", a);
  a = good;
  a.n = 0;
  expect_refused("n = 0", a);
  a = good;
  a.n = -3;
  expect_refused("n = -3", a);
  a = good;
  a.kind = 4;
  expect_refused("kind = 4", a);
  a = good;
  a.kind = -1;
  expect_refused("kind = -1", a);
  a = good;
  a.ldx = F - 4;
  expect_refused("ldx < F", a);
  a = good;
  a.lddx = F + 2;
  expect_refused("lddx % 4 != 0", a);
  a = good;
  a.x = nullptr;
  expect_refused("x null", a);
  a = good;
  a.W = nullptr;
  expect_refused("W null", a);
  a = good;
  a.y = nullptr;
  expect_refused("targets null", a);
  a = good;
  a.dx = nullptr;
  expect_refused("dx null", a);
  a = good;
  a.dW = nullptr;
  expect_refused("dW null", a);
  a = good;
  a.out = nullptr;
  expect_refused("out null", a);
  a = good;
  a.ws = nullptr;
  expect_refused("workspace null", a);
  a = good;
  a.x = x + 1;
  expect_refused("x misaligned", a);

  if (es_margin_softmax_workspace(n, C) != (size_t)n * (C + 2) || es_margin_softmax_workspace(0, C) != 0 ||
      es_margin_softmax_workspace(n, 65) != 0) {
    std::printf("FAIL es_margin_softmax_workspace\n");
    ++failures;
  }
  for (float* p = base; p < out + 1; ++p)
    if (*p != 0.f) {
      std::printf("FAIL a refused call wrote to a buffer\n");
      ++failures;
      break;
    }
  std::printf(failures ? "%d check(s) failed\n" : "all refused, nothing written (%d failures)\n", failures);
  return failures ? 1 : 0;
}
