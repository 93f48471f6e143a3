// Host-side sanitizer harness ("-fsanitize=address builds on the CPU-side
// harness"): libmiattack's host code — the C ABI's argument validation, the error-string state,
// the kernel-variant table and the reduction-scratch bookkeeping — compiled with
// -Xarch_host -fsanitize=address,undefined (device code unchanged) and driven through the public
// entry points with valid and invalid arguments. Any heap / stack / UB error aborts the process.
// No kernel is launched: every call below fails validation before reaching the GPU, except the
// scratch reserve / release cycle, which runs only when a device is present (the GPU box).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../../include/miattack.h"

static int g_fail = 0;
#define EXPECT(cond, what)                                               \
  do {                                                                   \
    if (!(cond)) {                                                       \
      std::fprintf(stderr, "FAIL %s (%s:%d)\n", what, __FILE__, __LINE__); \
      ++g_fail;                                                          \
    }                                                                    \
  } while (0)

static void expect_error(int rc, const char* what) {
  EXPECT(rc != MIA_OK, what);
  const char* msg = mia_last_error_string();
  EXPECT(msg != nullptr && std::strlen(msg) > 0, what);
}

// refused, and with this text in the message
static void expect_message(int rc, const char* text, const char* what) {
  EXPECT(rc != MIA_OK, what);
  const char* msg = mia_last_error_string();
  EXPECT(msg != nullptr && std::strstr(msg, text) != nullptr, what);
}

int main() {
  EXPECT(mia_version() > 0, "version");
  // tuning table: every documented switch round-trips; unknown / null names are refused
  const char* keys[] = {"MIA_CONV_HALO", "MIA_CONV_X6", "MIA_HALO_EPI", "MIA_X6_UNR",
                        "MIA_CONV_WRES128", "MIA_CONV_THIN", "MIA_CONV_THIN32", "MIA_CONV_WRES",
                        "MIA_CONV_REGEPI", "MIA_CONV_SMALLTILE", "MIA_S2DG_X6",
                        "MIA_S2DG_HALO", "MIA_UPCONV_X6", "MIA_UPCONV_HALO",
                        "MIA_CONV_WRES32", "MIA_HALO_C64", "MIA_X6_64S", "MIA_UPCONV_X6S"};
  for (const char* k : keys) {
    int v = -1, w = -1;
    EXPECT(mia_get_tuning(k, &v) == MIA_OK, k);
    EXPECT(mia_set_tuning(k, v + 7) == MIA_OK && mia_get_tuning(k, &w) == MIA_OK && w == v + 7, k);
    EXPECT(mia_set_tuning(k, v) == MIA_OK, k);
  }
  int v = 0;
  expect_error(mia_get_tuning("MIA_NO_SUCH_SWITCH", &v), "unknown switch");
  expect_error(mia_get_tuning("MIA_THIN_F32", &v), "removed switch");  // round 6
  expect_error(mia_get_tuning("MIA_EPI_PRERED", &v), "removed switch");
  expect_error(mia_set_tuning(nullptr, 1), "null switch");
  expect_error(mia_get_tuning("MIA_CONV_X6", nullptr), "null out");
  std::string longname(5000, 'x');  // the error string grows to hold it
  expect_error(mia_set_tuning(longname.c_str(), 1), "long name");
  EXPECT(std::strstr(mia_last_error_string(), "xxxx") != nullptr, "long name in error string");

  // workspace queries at the edges
  EXPECT(mia_conv_workspace_size(0, 16, 16, 64, 1) == 0, "ws N=0");
  EXPECT(mia_conv_workspace_size(2, 16, 16, 64, 0) == 0, "ws no sums");
  EXPECT(mia_conv_workspace_size(128, 1024, 1024, 32, 1) > 0, "ws 1024²");
  EXPECT(mia_conv_workspace_size(3, 7, 5, 8, 1) > 0, "ws ragged");
  EXPECT(mia_reduction_workspace_size(-1, 4, 4) == 0, "red ws");
  EXPECT(mia_ssim_workspace_size(2, 6, 6) == 0 && mia_ssim_workspace_size(3, 40, 37) > 0, "ssim ws");
  EXPECT(mia_conv_kpad(64, MIA_F16) >= 9 * 64 && mia_conv_kpad(3, MIA_F32) >= 27, "kpad");

  // argument validation of the conv entry points (no launch happens)
  expect_error(mia_conv3x3(nullptr, MIA_F32, nullptr), "conv3x3 null");
  mia_conv_args a;
  std::memset(&a, 0, sizeof(a));
  float dummy[64];
  a.x = a.w = a.y = dummy;
  a.N = 2; a.H = 16; a.W = 16; a.Cin = 64; a.Cout = 64;
  a.Kpad = mia_conv_kpad(64, MIA_F16) + 8;  // wrong
  expect_error(mia_conv3x3(&a, MIA_F16, nullptr), "conv3x3 bad Kpad");
  a.Kpad = mia_conv_kpad(64, MIA_F16);
  a.Cin = 48;  // not a power of two
  expect_error(mia_conv3x3(&a, MIA_F16, nullptr), "conv3x3 Cin");
  a.Cin = 64;
  a.sdot = dummy;  // sdot without aux_x
  expect_error(mia_conv3x3(&a, MIA_F16, nullptr), "conv3x3 sdot");
  a.sdot = nullptr;
  expect_error(mia_conv3x3(&a, 99, nullptr), "conv3x3 dtype");
  a.N = 1 << 20; a.H = 4096; a.W = 4096;  // 32-bit offset overflow guard
  expect_error(mia_conv3x3(&a, MIA_F16, nullptr), "conv3x3 size");
  a.N = 2; a.H = 16; a.W = 16;
  expect_error(mia_conv2d(&a, 3, nullptr, 1, 8, 8, MIA_F16, nullptr), "conv2d stride");
  expect_error(mia_conv2d(&a, 1, nullptr, 5, 8, 8, MIA_F16, nullptr), "conv2d groups");
  expect_error(mia_conv3x3_wmod(&a, 0, MIA_F16, nullptr), "wmod stride");
  expect_error(mia_conv3x3_wmod(&a, (int64_t)a.Cout * a.Kpad, MIA_F32, nullptr), "wmod fp32");
  a.in_scale = dummy;
  expect_error(mia_conv3x3_wmod(&a, (int64_t)a.Cout * a.Kpad, MIA_F16, nullptr), "wmod in_scale");
  expect_error(mia_modulate_weights(dummy, dummy, nullptr, dummy, 2, 64, 48, 9 * 48, MIA_F16,
                                    nullptr), "modw Cin");
  expect_error(mia_modulate_weights(nullptr, dummy, nullptr, dummy, 2, 64, 64,
                                    mia_conv_kpad(64, MIA_F16), MIA_F16, nullptr), "modw null");
  expect_error(mia_ssim2(dummy, dummy, 1, 5, 5, 2.f, nullptr, 0, dummy, nullptr), "ssim small");
  expect_error(mia_ssim2(dummy, dummy, 1, 64, 64, 0.f, (double*)dummy, 1 << 20, dummy, nullptr),
               "ssim dr");
  expect_error(mia_ssim2(dummy, dummy, 4, 64, 64, 2.f, (double*)dummy, 8 * 4, dummy, nullptr),
               "ssim work size");  // the round-3 contract (N doubles) is rejected
  expect_error(mia_gemm_f32_grouped(nullptr, 0, nullptr), "gemm groups");
  // the §8(b)-named K10 pair (round 6): nothing to write, or a 2-byte accumulating gradient
  expect_error(mia_mse_fwd_bwd(dummy, dummy, nullptr, nullptr, 1, 64, 1.f, 1.f, 0, MIA_F32,
                               nullptr), "mse_fwd_bwd no output");
  expect_error(mia_mse_fwd_bwd(dummy, dummy, dummy, dummy, 1, 64, 1.f, 1.f, 1, MIA_F16, nullptr),
               "mse_fwd_bwd fp16 accumulate");
  // the L2-ball PGD / momentum updates: null pointers, empty batches, shapes that do not fit
  expect_error(mia_grad_assemble_norms(nullptr, dummy, nullptr, nullptr, dummy, dummy, dummy, 2,
                                       32, 1, 8, 16, 1.f, 1.f, nullptr, MIA_F32, nullptr),
               "grad_assemble_norms null x");
  expect_error(mia_grad_assemble_norms(dummy, dummy, nullptr, nullptr, dummy, dummy, dummy, 0, 32,
                                       1, 8, 16, 1.f, 1.f, nullptr, MIA_F32, nullptr),
               "grad_assemble_norms N");
  expect_error(mia_grad_assemble_norms(dummy, dummy, dummy, nullptr, dummy, dummy, dummy, 2, 32, 3,
                                       8, 16, 1.f, 1.f, nullptr, MIA_F32, nullptr),
               "grad_assemble_norms pf");
  expect_error(mia_grad_assemble_norms(dummy, dummy, nullptr, dummy, dummy, dummy, dummy, 2, 32, 1,
                                       8, 5, 1.f, 1.f, nullptr, MIA_F32, nullptr),
               "grad_assemble_norms enc_res");
  expect_error(mia_grad_assemble_norms(dummy, dummy, nullptr, nullptr, dummy, dummy, dummy, 2, 32,
                                       1, 8, 16, 1.f, 1.f, nullptr, 99, nullptr),
               "grad_assemble_norms dtype");
  // the L∞ update, the plain assembly and the reconstruction's image gradient: the same checks
  expect_error(mia_pgd_update(dummy, nullptr, dummy, dummy, 2, 32, 1, 8, 16, 0.37f, 0.03f, 0.06f,
                              -1.f, 1.f, nullptr, MIA_F32, nullptr), "pgd_update null x0");
  expect_error(mia_pgd_update(dummy, dummy, dummy, dummy, 2, 32, 1, 2, 16, 0.37f, 0.03f, 0.06f,
                              -1.f, 1.f, nullptr, MIA_F32, nullptr), "pgd_update cpad");
  expect_error(mia_pgd_update(dummy, dummy, dummy, dummy, 1 << 16, 32, 1, 8, 16, 0.37f, 0.03f,
                              0.06f, -1.f, 1.f, nullptr, MIA_F32, nullptr), "pgd_update N");
  expect_error(mia_pgd_update(dummy, dummy, dummy, dummy, 2, 32, 1, 8, 0, 0.37f, 0.03f, 0.06f,
                              -1.f, 1.f, nullptr, MIA_F32, nullptr), "pgd_update enc_res");
  expect_error(mia_pgd_update(dummy, dummy, dummy, dummy, 2, 32, 1, 8, 16, 0.37f, 0.03f, 0.06f,
                              1.f, -1.f, nullptr, MIA_F32, nullptr), "pgd_update lo > hi");
  expect_error(mia_grad_assemble(dummy, dummy, dummy, dummy, nullptr, 2, 32, 1, 8, 16, 0.37f, 1.f,
                                 nullptr, MIA_F32, nullptr), "grad_assemble null g");
  expect_error(mia_grad_assemble(dummy, dummy, dummy, dummy, dummy, 2, 32, 1, 1, 16, 0.37f, 1.f,
                                 nullptr, MIA_F16, nullptr), "grad_assemble cpad");
  expect_error(mia_grad_assemble(dummy, dummy, dummy, dummy, dummy, 2, 32, 1, 8, 0, 0.37f, 1.f,
                                 nullptr, MIA_F32, nullptr), "grad_assemble enc_res 0");
  expect_error(mia_grad_assemble(dummy, dummy, dummy, dummy, dummy, 2, 20000, 1, 8, 16, 0.37f,
                                 1.f, nullptr, MIA_F32, nullptr), "grad_assemble S");
  expect_error(mia_image_grad(dummy, dummy, dummy, nullptr, 2, 32, 1, 8, 0.37f, MIA_F32, nullptr),
               "image_grad null g_img");
  expect_error(mia_image_grad(dummy, dummy, dummy, dummy, 2, 32, 3, 8, 0.37f, MIA_F32, nullptr),
               "image_grad pf");
  expect_error(mia_image_grad(dummy, dummy, dummy, dummy, 2, 32, 1, 2, 0.37f, MIA_BF16, nullptr),
               "image_grad cpad");
  expect_error(mia_image_grad(dummy, dummy, dummy, dummy, 0, 32, 1, 8, 0.37f, MIA_F32, nullptr),
               "image_grad N");
  expect_error(mia_image_grad(dummy, dummy, nullptr, dummy, 2, 32, 1, 8, 0.37f, 99, nullptr),
               "image_grad dtype");
  expect_error(mia_l2_step(dummy, dummy, dummy, nullptr, dummy, 2, 3072, 0.1f, nullptr, nullptr),
               "l2_step null norm");
  expect_error(mia_l2_step(dummy, dummy, dummy, dummy, dummy, -1, 3072, 0.1f, nullptr, nullptr),
               "l2_step N");
  expect_error(mia_l2_step(dummy, dummy, dummy, dummy, dummy, 2, 0, 0.1f, nullptr, nullptr),
               "l2_step plane");
  expect_error(mia_l2_project(dummy, nullptr, dummy, 2, 3072, 0.1f, -1.f, 1.f, nullptr),
               "l2_project null x0");
  expect_error(mia_l2_project(dummy, dummy, dummy, 2, 3072, 0.f, -1.f, 1.f, nullptr),
               "l2_project e");
  expect_error(mia_mi_update(dummy, dummy, dummy, dummy, nullptr, 2, 3072, 1.f, 0.1f, 0.1f, -1.f,
                             1.f, nullptr, nullptr), "mi_update null m");
  expect_error(mia_mi_update(dummy, dummy, dummy, dummy, dummy, 2, 3072, -1.f, 0.1f, 0.1f, -1.f,
                             1.f, nullptr, nullptr), "mi_update mu");
  expect_error(mia_mi_update(dummy, dummy, dummy, dummy, dummy, 1 << 20, 3072, 1.f, 0.1f, 0.1f,
                             -1.f, 1.f, nullptr, nullptr), "mi_update N");
  // the translation-invariant blur: null / in-place buffers, kernel lengths, sizes that overflow
  expect_error(mia_ti_smooth_norms(dummy, dummy + 32, nullptr, 15, dummy, dummy, 2, 3, 32, 32,
                                   nullptr, nullptr), "ti_smooth_norms null taps");
  expect_error(mia_ti_smooth_norms(dummy, dummy, dummy, 15, dummy, dummy, 2, 3, 32, 32, nullptr,
                                   nullptr), "ti_smooth_norms in place");
  expect_error(mia_ti_smooth_norms(dummy, dummy + 32, dummy, 14, dummy, dummy, 2, 3, 32, 32,
                                   nullptr, nullptr), "ti_smooth_norms even K");
  expect_error(mia_ti_smooth_norms(dummy, dummy + 32, dummy, 65, dummy, dummy, 2, 3, 32, 32,
                                   nullptr, nullptr), "ti_smooth_norms K > 63");
  expect_error(mia_ti_smooth_norms(dummy, dummy + 32, dummy, 15, dummy, dummy, 2, 3, 1 << 30,
                                   1 << 30, nullptr, nullptr), "ti_smooth_norms H*W overflow");
  expect_error(mia_ti_smooth_norms(dummy, dummy + 32, dummy, 15, dummy, dummy, 1 << 20, 3, 32, 32,
                                   nullptr, nullptr), "ti_smooth_norms N");
  // input diversity: null / aliased / overlapping buffers, the window's geometry, sizes that
  // overflow (2 images of 3 × 4 × 4 = 96 floats per buffer: di_a and di_b are disjoint)
  float di_buf[256];
  float* di_a = di_buf;
  float* di_b = di_buf + 128;
  expect_error(mia_di_resize_pad(nullptr, di_b, 2, 3, 4, 3, 0, 1, nullptr), "di null x");
  expect_error(mia_di_resize_pad(di_a, nullptr, 2, 3, 4, 3, 0, 1, nullptr), "di null y");
  expect_error(mia_di_resize_pad(di_a, di_a, 2, 3, 4, 3, 0, 1, nullptr), "di in place");
  expect_error(mia_di_resize_pad(di_a, di_a + 95, 2, 3, 4, 3, 0, 1, nullptr), "di overlap");
  expect_error(mia_di_resize_pad(di_a + 1, di_a, 2, 3, 4, 3, 0, 1, nullptr), "di overlap back");
  expect_error(mia_di_resize_pad(di_a, di_b, 2, 3, 4, 0, 0, 0, nullptr), "di rnd 0");
  expect_error(mia_di_resize_pad(di_a, di_b, 2, 3, 4, 5, 0, 0, nullptr), "di rnd > S");
  expect_error(mia_di_resize_pad(di_a, di_b, 2, 3, 4, 3, 2, 0, nullptr), "di top + rnd > S");
  expect_error(mia_di_resize_pad(di_a, di_b, 2, 3, 4, 3, 0, 2, nullptr), "di left + rnd > S");
  expect_error(mia_di_resize_pad(di_a, di_b, 2, 3, 4, 3, -1, 0, nullptr), "di top < 0");
  expect_error(mia_di_resize_pad(di_a, di_b, 2, 3, 4, 3, 0, 2147483647, nullptr),
               "di left + rnd overflows");
  expect_error(mia_di_resize_pad(di_a, di_b, 0, 3, 4, 3, 0, 1, nullptr), "di N 0");
  expect_error(mia_di_resize_pad(di_a, di_b, 1 << 16, 3, 4, 3, 0, 1, nullptr), "di N");
  expect_error(mia_di_resize_pad(di_a, di_b, 2, 0, 4, 3, 0, 1, nullptr), "di C 0");
  expect_error(mia_di_resize_pad(di_a, di_b, 2, 2, 1 << 15, 3, 0, 1, nullptr), "di C*S*S = 2^31");
  expect_error(mia_di_resize_pad(di_a, di_b, 2, 1, 1 << 16, 3, 0, 1, nullptr), "di S*S = 2^32");
  expect_error(mia_di_resize_pad_bwd_norms(nullptr, di_b, dummy, dummy, 2, 3, 4, 3, 0, 1, nullptr,
                                           nullptr), "di bwd null g");
  expect_error(mia_di_resize_pad_bwd_norms(di_a, nullptr, nullptr, nullptr, 2, 3, 4, 3, 0, 1,
                                           nullptr, nullptr), "di bwd null gx");
  expect_error(mia_di_resize_pad_bwd_norms(di_a, di_a, dummy, dummy, 2, 3, 4, 3, 0, 1, nullptr,
                                           nullptr), "di bwd in place");
  expect_error(mia_di_resize_pad_bwd_norms(di_a, di_a + 64, dummy, dummy, 2, 3, 4, 3, 0, 1,
                                           nullptr, nullptr), "di bwd overlap");
  expect_error(mia_di_resize_pad_bwd_norms(di_a, di_b, dummy, dummy, 2, 3, 4, 5, 0, 0, nullptr,
                                           nullptr), "di bwd rnd > S");
  expect_error(mia_di_resize_pad_bwd_norms(di_a, di_b, dummy, dummy, 2, 3, 4, 3, 2, 2, nullptr,
                                           nullptr), "di bwd window");
  expect_error(mia_di_resize_pad_bwd_norms(di_a, di_b, dummy, dummy, 70000, 3, 4, 3, 0, 1,
                                           nullptr, nullptr), "di bwd N");
  expect_error(mia_di_resize_pad_bwd_norms(di_a, di_b, dummy, dummy, 2, 3, 46341, 3, 0, 1,
                                           nullptr, nullptr), "di bwd S*S >= 2^31");
  // JPEG round trip and its adjoint: null / aliased / overlapping buffers, sizes that are no
  // multiple of 8 or overflow (1 image of 3 × 8 × 8 = 192 floats per buffer, a table of 128)
  static float jp_buf[4 * 192 + 128];
  float* jp_x = jp_buf;
  float* jp_y = jp_buf + 192;
  float* jp_g = jp_buf + 384;
  float* jp_q = jp_buf + 768;
  expect_error(mia_jpeg_roundtrip(nullptr, jp_y, jp_q, 1, 8, nullptr), "jpeg null x");
  expect_error(mia_jpeg_roundtrip(jp_x, nullptr, jp_q, 1, 8, nullptr), "jpeg null y");
  expect_error(mia_jpeg_roundtrip(jp_x, jp_y, nullptr, 1, 8, nullptr), "jpeg null qtab");
  expect_error(mia_jpeg_roundtrip(jp_x, jp_x, jp_q, 1, 8, nullptr), "jpeg in place");
  expect_error(mia_jpeg_roundtrip(jp_x, jp_x + 191, jp_q, 1, 8, nullptr), "jpeg overlap");
  expect_error(mia_jpeg_roundtrip(jp_x, jp_q - 191, jp_q, 1, 8, nullptr), "jpeg y over qtab");
  expect_error(mia_jpeg_roundtrip(jp_x, jp_y, jp_x + 64, 1, 8, nullptr), "jpeg qtab inside x");
  expect_error(mia_jpeg_roundtrip(jp_x, jp_y, jp_q, 1, 12, nullptr), "jpeg S = 12");
  expect_error(mia_jpeg_roundtrip(jp_x, jp_y, jp_q, 1, 4, nullptr), "jpeg S < 8");
  expect_error(mia_jpeg_roundtrip(jp_x, jp_y, jp_q, 1, 0, nullptr), "jpeg S 0");
  expect_error(mia_jpeg_roundtrip(jp_x, jp_y, jp_q, 1, -8, nullptr), "jpeg S < 0");
  expect_error(mia_jpeg_roundtrip(jp_x, jp_y, jp_q, 1, 26760, nullptr), "jpeg 3*S*S >= 2^31");
  expect_error(mia_jpeg_roundtrip(jp_x, jp_y, jp_q, 1, 1 << 30, nullptr), "jpeg S*S overflows");
  expect_error(mia_jpeg_roundtrip(jp_x, jp_y, jp_q, 0, 8, nullptr), "jpeg N 0");
  expect_error(mia_jpeg_roundtrip(jp_x, jp_y, jp_q, 1 << 16, 8, nullptr), "jpeg N");
  expect_error(mia_jpeg_bwd_norms(nullptr, jp_g, jp_y, jp_q, dummy, dummy, 1, 8, nullptr, nullptr),
               "jpeg bwd null x");
  expect_error(mia_jpeg_bwd_norms(jp_x, nullptr, jp_y, jp_q, dummy, dummy, 1, 8, nullptr, nullptr),
               "jpeg bwd null g");
  expect_error(mia_jpeg_bwd_norms(jp_x, jp_g, nullptr, jp_q, nullptr, nullptr, 1, 8, nullptr,
                                  nullptr), "jpeg bwd null gx");
  expect_error(mia_jpeg_bwd_norms(jp_x, jp_g, jp_y, nullptr, dummy, dummy, 1, 8, nullptr, nullptr),
               "jpeg bwd null qtab");
  expect_error(mia_jpeg_bwd_norms(jp_x, jp_g, jp_g, jp_q, dummy, dummy, 1, 8, nullptr, nullptr),
               "jpeg bwd in place");
  expect_error(mia_jpeg_bwd_norms(jp_x, jp_x, jp_y, jp_q, dummy, dummy, 1, 8, nullptr, nullptr),
               "jpeg bwd g is x");
  expect_error(mia_jpeg_bwd_norms(jp_x, jp_g, jp_x + 100, jp_q, dummy, dummy, 1, 8, nullptr,
                                  nullptr), "jpeg bwd gx over x");
  expect_error(mia_jpeg_bwd_norms(jp_x, jp_g, jp_y, jp_q, dummy, dummy, 1, 12, nullptr, nullptr),
               "jpeg bwd S = 12");
  expect_error(mia_jpeg_bwd_norms(jp_x, jp_g, jp_y, jp_q, dummy, dummy, 1, 26760, nullptr, nullptr),
               "jpeg bwd 3*S*S >= 2^31");
  expect_error(mia_jpeg_bwd_norms(jp_x, jp_g, jp_y, jp_q, dummy, dummy, 70000, 8, nullptr, nullptr),
               "jpeg bwd N");
  // scale copies / look-ahead: null / aliased / overlapping buffers, scales that are no 2^-i,
  // sizes (2 images of 48 floats per buffer: di_a and di_b are disjoint)
  expect_error(mia_si_transform(nullptr, nullptr, di_b, 2, 48, 0.f, 0.5f, nullptr), "si null x");
  expect_error(mia_si_transform(di_a, nullptr, nullptr, 2, 48, 0.f, 0.5f, nullptr), "si null y");
  expect_error(mia_si_transform(di_a, nullptr, di_a, 2, 48, 0.f, 0.5f, nullptr), "si in place");
  expect_error(mia_si_transform(di_a, nullptr, di_a + 95, 2, 48, 0.f, 0.5f, nullptr),
               "si overlap");
  expect_error(mia_si_transform(di_a, di_b, di_b, 2, 48, 0.f, 0.5f, nullptr), "si m is y");
  expect_error(mia_si_transform(di_a, di_b + 1, di_b, 2, 48, 0.f, 0.5f, nullptr),
               "si m overlaps y");
  expect_error(mia_si_transform(di_a, nullptr, di_b, 2, 48, 0.f, 0.75f, nullptr), "si s 0.75");
  expect_error(mia_si_transform(di_a, nullptr, di_b, 2, 48, 0.f, 2.f, nullptr), "si s 2");
  expect_error(mia_si_transform(di_a, nullptr, di_b, 2, 48, 0.f, 0.f, nullptr), "si s 0");
  expect_error(mia_si_transform(di_a, nullptr, di_b, 2, 48, 0.f, 0.00390625f, nullptr),
               "si s 2^-8");
  expect_error(mia_si_transform(di_a, nullptr, di_b, 2, 48, 0.f, nanf(""), nullptr), "si s nan");
  expect_error(mia_si_transform(di_a, nullptr, di_b, 2, 48, INFINITY, 0.5f, nullptr), "si c inf");
  expect_error(mia_si_transform(di_a, nullptr, di_b, 0, 48, 0.f, 0.5f, nullptr), "si N 0");
  expect_error(mia_si_transform(di_a, nullptr, di_b, 1 << 16, 48, 0.f, 0.5f, nullptr), "si N");
  expect_error(mia_si_transform(di_a, nullptr, di_b, 2, 0, 0.f, 0.5f, nullptr), "si plane 0");
  expect_error(mia_si_transform(di_a, nullptr, di_b, 2, 1LL << 31, 0.f, 0.5f, nullptr),
               "si plane 2^31");
  expect_error(mia_si_accumulate_norms(nullptr, di_b, dummy, dummy, 2, 48, 0.5f, 0, 1.f, nullptr,
                                       nullptr), "si acc null g");
  expect_error(mia_si_accumulate_norms(di_a, nullptr, nullptr, nullptr, 2, 48, 0.5f, 1, 1.f,
                                       nullptr, nullptr), "si acc null acc");
  expect_error(mia_si_accumulate_norms(di_a, di_a, dummy, dummy, 2, 48, 0.5f, 0, 1.f, nullptr,
                                       nullptr), "si acc in place");
  expect_error(mia_si_accumulate_norms(di_a, di_a + 64, dummy, dummy, 2, 48, 0.5f, 0, 1.f,
                                       nullptr, nullptr), "si acc overlap");
  expect_error(mia_si_accumulate_norms(di_a, di_b, dummy, dummy, 2, 48, 3.f, 0, 1.f, nullptr,
                                       nullptr), "si acc w 3");
  expect_error(mia_si_accumulate_norms(di_a, di_b, dummy, dummy, 2, 48, 0.5f, 0, 0.5f, nullptr,
                                       nullptr), "si acc div < 1");
  expect_error(mia_si_accumulate_norms(di_a, di_b, dummy, dummy, 2, 48, 0.5f, 0, nanf(""),
                                       nullptr, nullptr), "si acc div nan");
  expect_error(mia_si_accumulate_norms(di_a, di_b, dummy, dummy, 70000, 48, 0.5f, 0, 1.f,
                                       nullptr, nullptr), "si acc N");
  expect_error(mia_si_accumulate_norms(di_a, di_b, dummy, dummy, 2, -1, 0.5f, 0, 1.f, nullptr,
                                       nullptr), "si acc plane < 0");
  // SPSA: null / aliased / overlapping buffers, the probe radius, the scale, the divisor, sizes
  // and the image word (2 images of 48 floats per buffer: di_a, di_b and sp_c are disjoint;
  // sp_f holds fp at 0 and fm at 8)
  float sp_buf[128];
  float sp_f[16];
  float* sp_c = sp_buf;
  expect_error(mia_spsa_probe(nullptr, di_b, sp_c, 2, 48, 0.02f, -1.f, 1.f, 5, 0, 0, 0, nullptr),
               "spsa probe null x");
  expect_error(mia_spsa_probe(di_a, nullptr, sp_c, 2, 48, 0.02f, -1.f, 1.f, 5, 0, 0, 0, nullptr),
               "spsa probe null yp");
  expect_error(mia_spsa_probe(di_a, di_b, nullptr, 2, 48, 0.02f, -1.f, 1.f, 5, 0, 0, 0, nullptr),
               "spsa probe null ym");
  expect_error(mia_spsa_probe(di_a, di_a, sp_c, 2, 48, 0.02f, -1.f, 1.f, 5, 0, 0, 0, nullptr),
               "spsa probe yp is x");
  expect_error(mia_spsa_probe(di_a, di_b, di_a, 2, 48, 0.02f, -1.f, 1.f, 5, 0, 0, 0, nullptr),
               "spsa probe ym is x");
  expect_error(mia_spsa_probe(di_a, di_b, di_b, 2, 48, 0.02f, -1.f, 1.f, 5, 0, 0, 0, nullptr),
               "spsa probe ym is yp");
  expect_error(mia_spsa_probe(di_a, di_b, di_b + 95, 2, 48, 0.02f, -1.f, 1.f, 5, 0, 0, 0, nullptr),
               "spsa probe ym overlaps yp");
  expect_error(mia_spsa_probe(di_a + 1, di_a, sp_c, 2, 48, 0.02f, -1.f, 1.f, 5, 0, 0, 0, nullptr),
               "spsa probe overlap back");
  expect_error(mia_spsa_probe(di_a, di_b, sp_c, 2, 48, 0.f, -1.f, 1.f, 5, 0, 0, 0, nullptr),
               "spsa probe d 0");
  expect_error(mia_spsa_probe(di_a, di_b, sp_c, 2, 48, -0.02f, -1.f, 1.f, 5, 0, 0, 0, nullptr),
               "spsa probe d < 0");
  expect_error(mia_spsa_probe(di_a, di_b, sp_c, 2, 48, INFINITY, -1.f, 1.f, 5, 0, 0, 0, nullptr),
               "spsa probe d inf");
  expect_error(mia_spsa_probe(di_a, di_b, sp_c, 2, 48, nanf(""), -1.f, 1.f, 5, 0, 0, 0, nullptr),
               "spsa probe d nan");
  expect_error(mia_spsa_probe(di_a, di_b, sp_c, 2, 48, 0.02f, 1.f, -1.f, 5, 0, 0, 0, nullptr),
               "spsa probe lo > hi");
  expect_error(mia_spsa_probe(di_a, di_b, sp_c, 0, 48, 0.02f, -1.f, 1.f, 5, 0, 0, 0, nullptr),
               "spsa probe N 0");
  expect_error(mia_spsa_probe(di_a, di_b, sp_c, 1 << 16, 48, 0.02f, -1.f, 1.f, 5, 0, 0, 0,
                              nullptr), "spsa probe N");
  expect_error(mia_spsa_probe(di_a, di_b, sp_c, 2, 0, 0.02f, -1.f, 1.f, 5, 0, 0, 0, nullptr),
               "spsa probe plane 0");
  expect_error(mia_spsa_probe(di_a, di_b, sp_c, 2, 1LL << 31, 0.02f, -1.f, 1.f, 5, 0, 0, 0,
                              nullptr), "spsa probe plane 2^31");
  expect_error(mia_spsa_probe(di_a, di_b, sp_c, 2, 48, 0.02f, -1.f, 1.f, 5, 0xffffffffu, 0, 0,
                              nullptr), "spsa probe image0 + N > 2^32");
  expect_error(mia_spsa_accumulate_norms(nullptr, sp_f, sp_f + 8, dummy, dummy, 2, 48, 25.f, 5, 0,
                                         0, 0, 1, 1.f, nullptr, nullptr), "spsa acc null acc");
  expect_error(mia_spsa_accumulate_norms(di_a, nullptr, sp_f + 8, dummy, dummy, 2, 48, 25.f, 5, 0,
                                         0, 0, 1, 1.f, nullptr, nullptr), "spsa acc null fp");
  expect_error(mia_spsa_accumulate_norms(di_a, sp_f, nullptr, nullptr, nullptr, 2, 48, 25.f, 5, 0,
                                         0, 0, 1, 1.f, nullptr, nullptr), "spsa acc null fm");
  expect_error(mia_spsa_accumulate_norms(di_a, sp_f, sp_f, dummy, dummy, 2, 48, 25.f, 5, 0, 0, 0,
                                         1, 1.f, nullptr, nullptr), "spsa acc fm is fp");
  expect_error(mia_spsa_accumulate_norms(di_a, sp_f, sp_f + 1, dummy, dummy, 2, 48, 25.f, 5, 0, 0,
                                         0, 1, 1.f, nullptr, nullptr), "spsa acc fm overlaps fp");
  expect_error(mia_spsa_accumulate_norms(di_a, di_a + 95, sp_f, dummy, dummy, 2, 48, 25.f, 5, 0,
                                         0, 0, 1, 1.f, nullptr, nullptr), "spsa acc fp inside acc");
  expect_error(mia_spsa_accumulate_norms(di_a + 1, sp_f, di_a, dummy, dummy, 2, 48, 25.f, 5, 0, 0,
                                         0, 1, 1.f, nullptr, nullptr), "spsa acc inside fm");
  expect_error(mia_spsa_accumulate_norms(di_a, sp_f, sp_f + 8, dummy, dummy, 2, 48, 0.f, 5, 0, 0,
                                         0, 1, 1.f, nullptr, nullptr), "spsa acc s 0");
  expect_error(mia_spsa_accumulate_norms(di_a, sp_f, sp_f + 8, dummy, dummy, 2, 48, INFINITY, 5,
                                         0, 0, 0, 1, 1.f, nullptr, nullptr), "spsa acc s inf");
  expect_error(mia_spsa_accumulate_norms(di_a, sp_f, sp_f + 8, dummy, dummy, 2, 48, nanf(""), 5,
                                         0, 0, 0, 1, 1.f, nullptr, nullptr), "spsa acc s nan");
  expect_error(mia_spsa_accumulate_norms(di_a, sp_f, sp_f + 8, dummy, dummy, 2, 48, 25.f, 5, 0, 0,
                                         0, 1, 0.f, nullptr, nullptr), "spsa acc div 0");
  expect_error(mia_spsa_accumulate_norms(di_a, sp_f, sp_f + 8, dummy, dummy, 2, 48, 25.f, 5, 0, 0,
                                         0, 1, nanf(""), nullptr, nullptr), "spsa acc div nan");
  expect_error(mia_spsa_accumulate_norms(di_a, sp_f, sp_f + 8, dummy, dummy, 70000, 48, 25.f, 5,
                                         0, 0, 0, 1, 1.f, nullptr, nullptr), "spsa acc N");
  expect_error(mia_spsa_accumulate_norms(di_a, sp_f, sp_f + 8, dummy, dummy, 2, -1, 25.f, 5, 0, 0,
                                         0, 1, 1.f, nullptr, nullptr), "spsa acc plane < 0");
  expect_error(mia_spsa_accumulate_norms(di_a, sp_f, sp_f + 8, dummy, dummy, 2, 48, 25.f, 5,
                                         0xffffffffu, 0, 0, 1, 1.f, nullptr, nullptr),
               "spsa acc image0 + N > 2^32");
  // The universal perturbation: null / aliased / overlapping buffers, sizes, the range of the
  // integer sum, the step and the radius (2 images of 48 floats: g = di_a, x0 = di_b, x = sp_c,
  // l1 = sp_f; one plane of 48 for delta and acc)
  float up_d[48];
  int64_t up_acc[48];
  expect_error(mia_uap_accumulate(nullptr, sp_f, up_acc, 2, 48, 1, nullptr, nullptr),
               "uap acc null g");
  expect_error(mia_uap_accumulate(di_a, nullptr, up_acc, 2, 48, 1, nullptr, nullptr),
               "uap acc null l1");
  expect_error(mia_uap_accumulate(di_a, sp_f, nullptr, 2, 48, 1, nullptr, nullptr),
               "uap acc null acc");
  expect_error(mia_uap_accumulate(di_a, sp_f, (int64_t*)di_a, 2, 48, 1, nullptr, nullptr),
               "uap acc is g");
  expect_error(mia_uap_accumulate(di_a, sp_f, (int64_t*)(di_a + 94), 2, 48, 1, nullptr, nullptr),
               "uap acc inside g");
  expect_error(mia_uap_accumulate(di_a, (const float*)(up_acc + 47), up_acc, 2, 48, 1, nullptr,
                                  nullptr), "uap l1 inside acc");
  expect_error(mia_uap_accumulate(di_a, di_a + 95, up_acc, 2, 48, 1, nullptr, nullptr),
               "uap l1 inside g");
  expect_error(mia_uap_accumulate(di_a, sp_f, up_acc, 2, 48, 1, (int*)sp_f, nullptr),
               "uap nonfinite is l1");
  expect_error(mia_uap_accumulate(di_a, sp_f, (int64_t*)((char*)up_acc + 4), 2, 48, 1, nullptr,
                                  nullptr), "uap acc misaligned");
  expect_error(mia_uap_accumulate(di_a, sp_f, up_acc, 0, 48, 1, nullptr, nullptr), "uap acc N 0");
  expect_error(mia_uap_accumulate(di_a, sp_f, up_acc, 1 << 16, 48, 1, nullptr, nullptr),
               "uap acc N");
  expect_error(mia_uap_accumulate(di_a, sp_f, up_acc, 2, 0, 1, nullptr, nullptr),
               "uap acc plane 0");
  expect_error(mia_uap_accumulate(di_a, sp_f, up_acc, 2, 1LL << 31, 1, nullptr, nullptr),
               "uap acc plane 2^31");
  expect_error(mia_uap_accumulate(di_a, sp_f, up_acc, 65, (1LL << 31) - 1, 1, nullptr, nullptr),
               "uap acc N * plane >= 2^37");
  expect_error(mia_uap_step(nullptr, up_acc, sp_c, di_b, 2, 48, 0.01f, 0.06f, -1.f, 1.f, nullptr),
               "uap step null delta");
  expect_error(mia_uap_step(up_d, up_acc, nullptr, di_b, 2, 48, 0.01f, 0.06f, -1.f, 1.f, nullptr),
               "uap step null x");
  expect_error(mia_uap_step(up_d, up_acc, sp_c, nullptr, 2, 48, 0.01f, 0.06f, -1.f, 1.f, nullptr),
               "uap step null x0");
  expect_error(mia_uap_step(up_d, up_acc, sp_c, di_b, 0, 48, 0.01f, 0.06f, -1.f, 1.f, nullptr),
               "uap step N 0 with images");
  expect_error(mia_uap_step(up_d, nullptr, nullptr, nullptr, 0, 48, 0.01f, 0.06f, -1.f, 1.f,
                            nullptr), "uap step nothing to do");
  expect_error(mia_uap_step(up_d, up_acc, sp_c, di_b, -1, 48, 0.01f, 0.06f, -1.f, 1.f, nullptr),
               "uap step N < 0");
  expect_error(mia_uap_step(up_d, up_acc, sp_c, di_b, 1 << 16, 48, 0.01f, 0.06f, -1.f, 1.f,
                            nullptr), "uap step N");
  expect_error(mia_uap_step(up_d, up_acc, sp_c, di_b, 2, 0, 0.01f, 0.06f, -1.f, 1.f, nullptr),
               "uap step plane 0");
  expect_error(mia_uap_step(up_d, up_acc, sp_c, di_b, 2, 1LL << 31, 0.01f, 0.06f, -1.f, 1.f,
                            nullptr), "uap step plane 2^31");
  expect_error(mia_uap_step(up_d, (const int64_t*)up_d, sp_c, di_b, 2, 48, 0.01f, 0.06f, -1.f,
                            1.f, nullptr), "uap step acc is delta");
  expect_error(mia_uap_step(up_d, (const int64_t*)((char*)up_acc + 4), sp_c, di_b, 2, 48, 0.01f,
                            0.06f, -1.f, 1.f, nullptr), "uap step acc misaligned");
  expect_error(mia_uap_step(up_d, up_acc, di_b, di_b, 2, 48, 0.01f, 0.06f, -1.f, 1.f, nullptr),
               "uap step x is x0");
  expect_error(mia_uap_step(up_d, up_acc, di_b + 95, di_b, 2, 48, 0.01f, 0.06f, -1.f, 1.f,
                            nullptr), "uap step x overlaps x0");
  expect_error(mia_uap_step(up_d, up_acc, up_d, di_b, 2, 48, 0.01f, 0.06f, -1.f, 1.f, nullptr),
               "uap step x is delta");
  expect_error(mia_uap_step(up_d, up_acc, sp_c, up_d + 47, 2, 48, 0.01f, 0.06f, -1.f, 1.f,
                            nullptr), "uap step x0 inside delta");
  expect_error(mia_uap_step(up_d, up_acc, (float*)up_acc, di_b, 2, 48, 0.01f, 0.06f, -1.f, 1.f,
                            nullptr), "uap step x is acc");
  expect_error(mia_uap_step(up_d, up_acc, sp_c, di_b, 2, 48, -0.01f, 0.06f, -1.f, 1.f, nullptr),
               "uap step a < 0");
  expect_error(mia_uap_step(up_d, up_acc, sp_c, di_b, 2, 48, nanf(""), 0.06f, -1.f, 1.f, nullptr),
               "uap step a nan");
  expect_error(mia_uap_step(up_d, up_acc, sp_c, di_b, 2, 48, 0.01f, 0.f, -1.f, 1.f, nullptr),
               "uap step e 0");
  expect_error(mia_uap_step(up_d, up_acc, sp_c, di_b, 2, 48, 0.01f, nanf(""), -1.f, 1.f, nullptr),
               "uap step e nan");
  expect_error(mia_uap_step(up_d, up_acc, sp_c, di_b, 2, 48, 0.01f, 0.06f, 1.f, -1.f, nullptr),
               "uap step lo > hi");
  // SignHunter: null / aliased / overlapping buffers, sizes, the two ranges, the radius and the
  // bounds (2 images of 48 elements: x = sp_c, x0 = di_b, s = sh_s, accept = sh_i; the decision's
  // arrays of 2 words each: loss = sp_f, best = sp_f + 2, hist = sp_f + 4, accept = sh_i,
  // n_accept = sh_i + 2, nonfinite = sh_i + 4)
  int8_t sh_s[96];
  int sh_i[8];
  expect_error(mia_sh_flip(nullptr, di_b, sh_s, sh_i, 2, 48, 0, 24, 24, 48, 0.06f, -1.f, 1.f,
                           nullptr), "sh flip null x");
  expect_error(mia_sh_flip(sp_c, nullptr, sh_s, sh_i, 2, 48, 0, 24, 24, 48, 0.06f, -1.f, 1.f,
                           nullptr), "sh flip null x0");
  expect_error(mia_sh_flip(sp_c, di_b, nullptr, nullptr, 2, 48, 0, 24, 24, 48, 0.06f, -1.f, 1.f,
                           nullptr), "sh flip null s");
  expect_error(mia_sh_flip(sp_c, sp_c, sh_s, sh_i, 2, 48, 0, 24, 24, 48, 0.06f, -1.f, 1.f,
                           nullptr), "sh flip x0 is x");
  expect_error(mia_sh_flip(sp_c, sp_c + 95, sh_s, sh_i, 2, 48, 0, 24, 24, 48, 0.06f, -1.f, 1.f,
                           nullptr), "sh flip x0 overlaps x");
  expect_error(mia_sh_flip(sp_c, di_b, (int8_t*)sp_c + 383, sh_i, 2, 48, 0, 24, 24, 48, 0.06f,
                           -1.f, 1.f, nullptr), "sh flip s at x's last byte");
  expect_error(mia_sh_flip(sp_c, (const float*)(sh_s + 95), sh_s, sh_i, 2, 48, 0, 24, 24, 48,
                           0.06f, -1.f, 1.f, nullptr), "sh flip x0 at s's last byte");
  expect_error(mia_sh_flip(sp_c, di_b, sh_s, (const int*)(sp_c + 95), 2, 48, 0, 24, 24, 48, 0.06f,
                           -1.f, 1.f, nullptr), "sh flip accept inside x");
  expect_error(mia_sh_flip(sp_c, di_b, sh_s, (const int*)(sh_s + 92), 2, 48, 0, 24, 24, 48, 0.06f,
                           -1.f, 1.f, nullptr), "sh flip accept inside s");
  expect_error(mia_sh_flip(sp_c, di_b, sh_s, sh_i, 0, 48, 0, 24, 24, 48, 0.06f, -1.f, 1.f,
                           nullptr), "sh flip N 0");
  expect_error(mia_sh_flip(sp_c, di_b, sh_s, sh_i, 1 << 16, 48, 0, 24, 24, 48, 0.06f, -1.f, 1.f,
                           nullptr), "sh flip N");
  expect_error(mia_sh_flip(sp_c, di_b, sh_s, sh_i, 2, 0, 0, 0, 0, 0, 0.06f, -1.f, 1.f, nullptr),
               "sh flip plane 0");
  expect_error(mia_sh_flip(sp_c, di_b, sh_s, sh_i, 2, 1LL << 31, 0, 24, 24, 48, 0.06f, -1.f, 1.f,
                           nullptr), "sh flip plane 2^31");
  expect_error(mia_sh_flip(sp_c, di_b, sh_s, sh_i, 2, 48, -1, 24, 24, 48, 0.06f, -1.f, 1.f,
                           nullptr), "sh flip prev_lo < 0");
  expect_error(mia_sh_flip(sp_c, di_b, sh_s, sh_i, 2, 48, 25, 24, 24, 48, 0.06f, -1.f, 1.f,
                           nullptr), "sh flip prev_lo > prev_hi");
  expect_error(mia_sh_flip(sp_c, di_b, sh_s, sh_i, 2, 48, 0, 49, 24, 48, 0.06f, -1.f, 1.f,
                           nullptr), "sh flip prev_hi > plane");
  expect_error(mia_sh_flip(sp_c, di_b, sh_s, sh_i, 2, 48, 0, 24, -2, 48, 0.06f, -1.f, 1.f,
                           nullptr), "sh flip lo < 0");
  expect_error(mia_sh_flip(sp_c, di_b, sh_s, sh_i, 2, 48, 0, 24, 30, 29, 0.06f, -1.f, 1.f,
                           nullptr), "sh flip lo > hi");
  expect_error(mia_sh_flip(sp_c, di_b, sh_s, sh_i, 2, 48, 0, 24, 24, 49, 0.06f, -1.f, 1.f,
                           nullptr), "sh flip hi > plane");
  expect_error(mia_sh_flip(sp_c, di_b, sh_s, sh_i, 2, 48, 7, 7, 48, 48, 0.06f, -1.f, 1.f,
                           nullptr), "sh flip both ranges empty");
  expect_error(mia_sh_flip(sp_c, di_b, sh_s, nullptr, 2, 48, 0, 0, 0, 0, 0.06f, -1.f, 1.f,
                           nullptr), "sh flip both ranges empty, no accept");
  expect_error(mia_sh_flip(sp_c, di_b, sh_s, sh_i, 2, 48, 0, 24, 24, 48, 0.f, -1.f, 1.f, nullptr),
               "sh flip e 0");
  expect_error(mia_sh_flip(sp_c, di_b, sh_s, sh_i, 2, 48, 0, 24, 24, 48, -0.06f, -1.f, 1.f,
                           nullptr), "sh flip e < 0");
  expect_error(mia_sh_flip(sp_c, di_b, sh_s, sh_i, 2, 48, 0, 24, 24, 48, INFINITY, -1.f, 1.f,
                           nullptr), "sh flip e inf");
  expect_error(mia_sh_flip(sp_c, di_b, sh_s, sh_i, 2, 48, 0, 24, 24, 48, nanf(""), -1.f, 1.f,
                           nullptr), "sh flip e nan");
  expect_error(mia_sh_flip(sp_c, di_b, sh_s, sh_i, 2, 48, 0, 24, 24, 48, 0.06f, 1.f, -1.f,
                           nullptr), "sh flip lo_v > hi_v");
  expect_error(mia_sh_flip(sp_c, di_b, sh_s, sh_i, 2, 48, 0, 24, 24, 48, 0.06f, nanf(""), 1.f,
                           nullptr), "sh flip lo_v nan");
  expect_error(mia_sh_decide(nullptr, sp_f + 2, sh_i, sh_i + 2, sp_f + 4, 2, 0, sh_i + 4, nullptr),
               "sh decide null loss");
  expect_error(mia_sh_decide(sp_f, nullptr, sh_i, sh_i + 2, sp_f + 4, 2, 0, sh_i + 4, nullptr),
               "sh decide null best");
  expect_error(mia_sh_decide(sp_f, sp_f + 2, nullptr, sh_i + 2, sp_f + 4, 2, 0, nullptr, nullptr),
               "sh decide null accept");
  expect_error(mia_sh_decide(sp_f, sp_f + 2, sh_i, nullptr, sp_f + 4, 2, 0, sh_i + 4, nullptr),
               "sh decide null n_accept");
  expect_error(mia_sh_decide(sp_f, sp_f + 2, sh_i, sh_i + 2, nullptr, 2, 1, sh_i + 4, nullptr),
               "sh decide null hist");
  expect_error(mia_sh_decide(sp_f, sp_f, sh_i, sh_i + 2, sp_f + 4, 2, 0, sh_i + 4, nullptr),
               "sh decide best is loss");
  expect_error(mia_sh_decide(sp_f, sp_f + 1, sh_i, sh_i + 2, sp_f + 4, 2, 0, sh_i + 4, nullptr),
               "sh decide best overlaps loss");
  expect_error(mia_sh_decide(sp_f, sp_f + 2, sh_i, sh_i + 1, sp_f + 4, 2, 0, sh_i + 4, nullptr),
               "sh decide n_accept overlaps accept");
  expect_error(mia_sh_decide(sp_f, sp_f + 2, sh_i, sh_i + 2, sp_f + 3, 2, 0, sh_i + 4, nullptr),
               "sh decide hist overlaps best");
  expect_error(mia_sh_decide(sp_f, sp_f + 2, sh_i, sh_i + 2, sp_f + 4, 2, 0, sh_i + 3, nullptr),
               "sh decide nonfinite overlaps n_accept");
  expect_error(mia_sh_decide(sp_f, sp_f + 2, sh_i, sh_i + 2, sp_f + 4, 2, 0, (int*)sp_f, nullptr),
               "sh decide nonfinite is loss");
  expect_error(mia_sh_decide(sp_f, sp_f + 2, sh_i, sh_i + 2, sp_f + 4, 0, 0, sh_i + 4, nullptr),
               "sh decide N 0");
  expect_error(mia_sh_decide(sp_f, sp_f + 2, sh_i, sh_i + 2, sp_f + 4, 1 << 16, 0, sh_i + 4,
                             nullptr), "sh decide N");
  expect_error(mia_sh_decide(sp_f, sp_f + 2, sh_i, sh_i + 2, sp_f + 4, 2, 2, sh_i + 4, nullptr),
               "sh decide first 2");
  expect_error(mia_sh_decide(sp_f, sp_f + 2, sh_i, sh_i + 2, sp_f + 4, 2, -1, sh_i + 4, nullptr),
               "sh decide first < 0");
  // Partial overlaps from each side (b starting inside a, and a starting inside b) of the entry
  // points whose buffers differ in length or element size, each refused with its own message.
  // Offsets in floats into one allocation; 2 images of 48 elements; nothing is dereferenced.
  alignas(16) static float ov[512];
  {
    const char* m = "acc, fp and fm must be distinct buffers";
    auto f = [&](int acc, int fp, int fm) {  // acc 96 floats, fp and fm 2 each
      return mia_spsa_accumulate_norms(ov + acc, ov + fp, ov + fm, dummy, dummy, 2, 48, 25.f, 5, 0,
                                       0, 0, 1, 1.f, nullptr, nullptr);
    };
    expect_message(f(0, 95, 200), m, "spsa acc: fp starts inside acc");
    expect_message(f(101, 100, 200), m, "spsa acc: acc starts inside fp");
    expect_message(f(0, 200, 95), m, "spsa acc: fm starts inside acc");
    expect_message(f(101, 200, 100), m, "spsa acc: acc starts inside fm");
    expect_message(f(0, 200, 201), m, "spsa acc: fm starts inside fp");
    expect_message(f(0, 201, 200), m, "spsa acc: fp starts inside fm");
  }
  {
    const char* m = "the state, action, loss and history arrays must be distinct buffers";
    auto f = [&](int fstate, int istate) {  // fstate 8 floats, istate 6 ints, the others 2 words
      return mia_apgd_decide(ov, ov + fstate, (int*)(ov + istate), (int*)(ov + 2), ov + 4, ov + 6, 2,
                             1, 0, 0, 0.f, nullptr);
    };
    expect_message(f(8, 15), m, "apgd decide: istate starts inside fstate");
    expect_message(f(13, 8), m, "apgd decide: fstate starts inside istate");
    expect_message(f(7, 20), m, "apgd decide: fstate starts inside hist_eta");
    expect_message(f(20, 3), m, "apgd decide: istate starts inside action");
  }
  {
    const char* m = "loss, best, accept, n_accept, hist_loss and nonfinite must be distinct buffers";
    auto f = [&](int loss, int best, int accept, int nonfinite) {  // 2 words each
      return mia_sh_decide(ov + loss, ov + best, (int*)(ov + accept), (int*)(ov + 20), ov + 30, 2, 0,
                           nonfinite < 0 ? nullptr : (int*)(ov + nonfinite), nullptr);
    };
    expect_message(f(0, 1, 10, 40), m, "sh decide: best starts inside loss");
    expect_message(f(1, 0, 10, 40), m, "sh decide: loss starts inside best");
    expect_message(f(0, 4, 10, 11), m, "sh decide: nonfinite starts inside accept");
    expect_message(f(0, 4, 11, 10), m, "sh decide: accept starts inside nonfinite");
    expect_message(f(0, 4, 1, -1), m, "sh decide: accept starts inside loss, no nonfinite");
  }
  {
    const char* m = "x, x0, s and accept must be distinct buffers";
    // x, x0 96 floats, s 96 bytes, accept 2 ints
    auto f = [&](int x, int x0, int s_bytes, int accept) {
      return mia_sh_flip(ov + x, ov + x0, (int8_t*)ov + s_bytes,
                         accept < 0 ? nullptr : (int*)(ov + accept), 2, 48, 0, 24, 24, 48, 0.06f, -1.f, 1.f, nullptr);
    };
    expect_message(f(0, 95, 4 * 300, 400), m, "sh flip: x0 starts inside x");
    expect_message(f(95, 0, 4 * 300, 400), m, "sh flip: x starts inside x0");
    expect_message(f(0, 100, 4 * 95 + 3, 400), m, "sh flip: s starts inside x");
    expect_message(f(323, 100, 4 * 300, 400), m, "sh flip: x starts inside s");
    expect_message(f(0, 100, 4 * 300, 323), m, "sh flip: accept starts inside s");
    expect_message(f(0, 100, 4 * 300 + 7, 300), m, "sh flip: s starts inside accept");
    expect_message(f(0, 100, 4 * 300, 195), m, "sh flip: accept starts inside x0");
    expect_message(f(0, 101, 4 * 300, 100), m, "sh flip: x0 starts inside accept");
    expect_message(f(0, 100, 4 * 95, -1), m, "sh flip: s starts inside x, no accept");
  }
  {
    const char* m = "g, l1, acc and nonfinite must be distinct buffers";
    // g 96 floats, l1 2, acc 48 int64, nonfinite 2 ints
    auto f = [&](int g, int l1, int acc, int nonfinite) {
      return mia_uap_accumulate(ov + g, ov + l1, (int64_t*)(ov + acc), 2, 48, 1,
                                nonfinite < 0 ? nullptr : (int*)(ov + nonfinite), nullptr);
    };
    expect_message(f(0, 300, 94, -1), m, "uap acc: acc starts inside g");
    expect_message(f(195, 300, 100, -1), m, "uap acc: g starts inside acc");
    expect_message(f(0, 195, 100, -1), m, "uap acc: l1 starts inside acc");
    expect_message(f(0, 99, 100, -1), m, "uap acc: acc starts inside l1");
    expect_message(f(0, 95, 100, -1), m, "uap acc: l1 starts inside g");
    expect_message(f(1, 0, 100, -1), m, "uap acc: g starts inside l1");
    expect_message(f(0, 300, 100, 195), m, "uap acc: nonfinite starts inside acc");
    expect_message(f(0, 300, 100, 99), m, "uap acc: acc starts inside nonfinite");
    expect_message(f(0, 300, 100, 301), m, "uap acc: nonfinite starts inside l1");
    expect_message(f(0, 301, 100, 300), m, "uap acc: l1 starts inside nonfinite");
  }
  {
    const char* m2 = "delta and acc must be distinct";
    const char* m4 = "delta, acc, x and x0 must be distinct buffers";
    // delta 48 floats, acc 48 int64, x and x0 96 floats
    auto f = [&](int delta, int acc, int x, int x0) {
      return mia_uap_step(ov + delta, (const int64_t*)(ov + acc), ov + x, ov + x0, 2, 48, 0.01f,
                          0.06f, -1.f, 1.f, nullptr);
    };
    expect_message(f(0, 46, 200, 300), m2, "uap step: acc starts inside delta");
    expect_message(f(195, 100, 200, 300), m2, "uap step: delta starts inside acc");
    expect_message(f(0, 100, 200, 295), m4, "uap step: x0 starts inside x");
    expect_message(f(0, 100, 295, 200), m4, "uap step: x starts inside x0");
    expect_message(f(0, 100, 195, 300), m4, "uap step: x starts inside acc");
    expect_message(f(0, 294, 200, 400), m4, "uap step: acc starts inside x");
    expect_message(f(0, 100, 200, 47), m4, "uap step: x0 starts inside delta");
    expect_message(f(295, 100, 300, 200), m4, "uap step: delta starts inside x0");
    expect_message(mia_uap_step(ov, (const int64_t*)(ov + 46), nullptr, nullptr, 0, 48, 0.01f, 0.06f,
                                -1.f, 1.f, nullptr), m2, "uap step: acc starts inside delta, N = 0");
  }
  // The patch-wise step: null / aliased / overlapping buffers (m and A ping-pong, never in
  // place), the kernel, the sizes and the scalars (2 images of 3 × 4 × 4 = 48 elements, 96 floats
  // per buffer: x, x0, g, m_in, m_out, A_in, A_out = pi_b[0 … 6]; l1 = pi_l1)
  float pi_buf[7 * 96], pi_l1[2];
  float* pi_b[7];
  for (int i = 0; i < 7; ++i) pi_b[i] = pi_buf + 96 * i;
  auto pi = [&](float* x, const float* x0, const float* g, const float* l1, const float* m_in,
                float* m_out, const float* A_in, float* A_out, int N = 2, int C = 3, int H = 4,
                int W = 4, int K = 3, float mu = 1.f, float ab = 0.1f, float gm = 0.1f,
                float e = 0.06f, float lo = -1.f, float hi = 1.f, int* nonfinite = nullptr) {
    return mia_pi_update(x, x0, g, l1, m_in, m_out, A_in, A_out, N, C, H, W, K, mu, ab, gm, e, lo,
                         hi, nonfinite, nullptr);
  };
  float *px = pi_b[0], *px0 = pi_b[1], *pg = pi_b[2], *pmi = pi_b[3], *pmo = pi_b[4],
        *pai = pi_b[5], *pao = pi_b[6];
  expect_error(pi(nullptr, px0, pg, pi_l1, pmi, pmo, pai, pao), "pi null x");
  expect_error(pi(px, nullptr, pg, pi_l1, pmi, pmo, pai, pao), "pi null x0");
  expect_error(pi(px, px0, nullptr, pi_l1, pmi, pmo, pai, pao), "pi null g");
  expect_error(pi(px, px0, pg, nullptr, pmi, pmo, pai, pao), "pi null l1");
  expect_error(pi(px, px0, pg, pi_l1, nullptr, pmo, pai, pao), "pi null m_in");
  expect_error(pi(px, px0, pg, pi_l1, pmi, nullptr, pai, pao), "pi null m_out");
  expect_error(pi(px, px0, pg, pi_l1, pmi, pmo, nullptr, pao), "pi null A_in");
  expect_error(pi(px, px0, pg, pi_l1, pmi, pmo, pai, nullptr), "pi null A_out");
  expect_error(pi(px, px0, pg, pi_l1, pmi, pmi, pai, pao), "pi m in place");
  expect_error(pi(px, px0, pg, pi_l1, pmi, pmo, pai, pai), "pi A in place");
  expect_error(pi(px, px0, pg, pi_l1, pmi, pmi + 95, pai, pao), "pi m_out overlaps m_in");
  expect_error(pi(px, px0, pg, pi_l1, pmo + 95, pmo, pai, pao), "pi m_in overlaps m_out");
  expect_error(pi(px, px0, pg, pi_l1, pmi, pmo, pai, pai + 1), "pi A_out overlaps A_in");
  expect_error(pi(px, px, pg, pi_l1, pmi, pmo, pai, pao), "pi x0 is x");
  expect_error(pi(px, px0, px + 95, pi_l1, pmi, pmo, pai, pao), "pi g overlaps x");
  expect_error(pi(px, px0, pg, pi_l1, pmi, px, pai, pao), "pi m_out is x");
  expect_error(pi(px, px0, pg, pi_l1, pmi, pmo, pai, pmo), "pi A_out is m_out");
  expect_error(pi(px, px0, pg, pi_l1, pmi, pmo, pmo + 95, pao), "pi A_in overlaps m_out");
  expect_error(pi(px, pao + 95, pg, pi_l1, pmi, pmo, pai, pao), "pi x0 overlaps A_out");
  expect_error(pi(px, px0, pg, px + 95, pmi, pmo, pai, pao), "pi l1 inside x");
  expect_error(pi(px, px0, pg, pao, pmi, pmo, pai, pao), "pi l1 is A_out");
  for (int K : {1, 2, 4, 16, 17, 63, 0, -3})
    expect_error(pi(px, px0, pg, pi_l1, pmi, pmo, pai, pao, 2, 3, 4, 4, K), "pi K");
  expect_error(pi(px, px0, pg, pi_l1, pmi, pmo, pai, pao, 0), "pi N 0");
  expect_error(pi(px, px0, pg, pi_l1, pmi, pmo, pai, pao, 1 << 16), "pi N");
  expect_error(pi(px, px0, pg, pi_l1, pmi, pmo, pai, pao, 2, 0), "pi C 0");
  expect_error(pi(px, px0, pg, pi_l1, pmi, pmo, pai, pao, 2, 3, 0), "pi H 0");
  expect_error(pi(px, px0, pg, pi_l1, pmi, pmo, pai, pao, 2, 3, 4, -4), "pi W < 0");
  expect_error(pi(px, px0, pg, pi_l1, pmi, pmo, pai, pao, 2, 1, 1 << 16, 1 << 15), "pi H·W 2^31");
  expect_error(pi(px, px0, pg, pi_l1, pmi, pmo, pai, pao, 2, 2, 1 << 15, 1 << 15), "pi plane 2^31");
  for (float v : {-0.5f, INFINITY, -INFINITY, nanf("")}) {
    expect_error(pi(px, px0, pg, pi_l1, pmi, pmo, pai, pao, 2, 3, 4, 4, 3, v), "pi mu");
    expect_error(pi(px, px0, pg, pi_l1, pmi, pmo, pai, pao, 2, 3, 4, 4, 3, 1.f, v), "pi ab");
    expect_error(pi(px, px0, pg, pi_l1, pmi, pmo, pai, pao, 2, 3, 4, 4, 3, 1.f, 0.1f, v), "pi gm");
    expect_error(pi(px, px0, pg, pi_l1, pmi, pmo, pai, pao, 2, 3, 4, 4, 3, 1.f, 0.1f, 0.1f, v),
                 "pi e");
  }
  expect_error(pi(px, px0, pg, pi_l1, pmi, pmo, pai, pao, 2, 3, 4, 4, 3, 1.f, 0.1f, 0.1f, 0.06f,
                  1.f, -1.f), "pi lo > hi");
  expect_error(pi(px, px0, pg, pi_l1, pmi, pmo, pai, pao, 2, 3, 4, 4, 3, 1.f, 0.1f, 0.1f, 0.06f,
                  nanf(""), 1.f), "pi lo nan");
  expect_error(mia_reserve_reduction_scratch(-1, nullptr), "scratch negative");
  EXPECT(mia_reserve_reduction_scratch(0, nullptr) == MIA_OK, "scratch zero");

  // the scratch table's grow / release cycle (device present only)
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) == hipSuccess && ndev > 0) {
    hipStream_t st;
    EXPECT(hipStreamCreate(&st) == hipSuccess, "stream");
    for (int64_t b : {int64_t(1) << 10, int64_t(1) << 22, int64_t(1) << 12, int64_t(1) << 24}) {
      EXPECT(mia_reserve_reduction_scratch(b, st) == MIA_OK, "reserve");
      EXPECT(mia_reduction_scratch_bytes(st) >= b, "reserved bytes");
    }
    EXPECT(mia_release_reduction_scratch(st) == MIA_OK, "release");
    EXPECT(mia_reduction_scratch_bytes(st) == 0, "released");
    EXPECT(mia_release_reduction_scratch(st) == MIA_OK, "release twice");
    (void)hipStreamDestroy(st);
    std::printf("scratch cycle on %d device(s): ok\n", ndev);
  } else {
    std::printf("no device: scratch cycle skipped\n");
  }
  std::printf("host ABI checks: %s (%d failures)\n", g_fail ? "FAILED" : "ok", g_fail);
  return g_fail ? 1 : 0;
}
