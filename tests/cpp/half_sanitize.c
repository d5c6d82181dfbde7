/*
 * half_sanitize.c — the half-precision-storage entry points' host code under
 * AddressSanitizer and UndefinedBehaviorSanitizer (device code untouched:
 * -Xarch_host only).  Built and run by tools/host_asan.sh beside
 * capi_sanitize.c, on a machine without a GPU: the storage switch over every
 * code, the refused flags, the argument checks of the step calls (null and
 * odd pointers, empty blocks, rows past the columns, launch index, semantics,
 * aliased v) and of the whole solves, with pointers that are never read - so
 * the validation, the error formatting and the offset arithmetic in front of
 * the launches run under the sanitizers.  With a device it also runs one
 * small host-pointer solve per storage format.
 * Exit 0 = clean.
 */
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "similarity_transform.h"

static int fails = 0;

#define CHECK(c)                                                                 \
  do {                                                                           \
    if (!(c)) {                                                                  \
      fprintf(stderr, "%s:%d: check failed: %s (%s)\n", __FILE__, __LINE__, #c,  \
              eigen_last_error());                                               \
      fails++;                                                                   \
    }                                                                            \
  } while (0)

static int
says(const char* what)
{
  return strstr(eigen_last_error(), what) != NULL;
}

/* bfloat16 / binary16 bit patterns of small integers 1 .. 8 (exact) */
static uint16_t
bf16_of(int i)
{
  const float f = (float)i;
  uint32_t b;
  memcpy(&b, &f, 4);
  return (uint16_t)(b >> 16);
}
static uint16_t
f16_of(int i)
{
  static const uint16_t t[9] = { 0,      0x3c00, 0x4000, 0x4200, 0x4400,
                                 0x4500, 0x4600, 0x4700, 0x4800 };
  return t[i];
}

int
main(void)
{
  setvbuf(stdout, NULL, _IONBF, 0); /* LeakSanitizer exits without a flush */
  void* const dummy = (void*)4096; /* refused before it could be read */
  void* const dummy2 = (void*)8192;
  float lam = 0, v[16];
  unsigned int it = 0;
  st_state* const st = (st_state*)dummy;

  /* the storage switch: 2 and 3 only, the message names the value */
  static const int bad_codes[] = { -1, 0, 1, 4, 255 };
  for (size_t i = 0; i < sizeof bad_codes / sizeof bad_codes[0]; i++) {
    const int c = bad_codes[i];
    char want[32];
    snprintf(want, sizeof want, "got %d", c);
    CHECK(st_rowsum_half(c, dummy, (float*)dummy, 4, 4, NULL) < 0 && says(want));
    CHECK(st_mfree_round_half(c, dummy, (float*)dummy, (float*)dummy, (float*)dummy,
                              (float*)dummy2, 4, 4, 0, 1e-3f, 1, 10, 0, st, NULL) < 0 &&
          says(want));
    CHECK(st_narrow_f32(c, (float*)dummy, dummy, 4, NULL) < 0 && says(want));
    CHECK(st_solve_device_half(dummy, c, dummy, 4, (float*)dummy, NULL, &lam, &it, NULL,
                               NULL) < 0 && says(want));
    CHECK(max_eigen_value_half_ex(dummy, c, dummy, &lam, v, 4, &it, NULL, NULL) < 0 &&
          says(want));
  }

  for (int c = ST_STORE_F16; c <= ST_STORE_BF16; c++) {
    /* the flags of the writing forms, alone and combined, before the queue */
    static const uint32_t refused[] = { 4u, 8u, 32u, 4u | 2u, 8u | 1u, 32u | 16u, 4u | 8u | 32u };
    for (size_t i = 0; i < sizeof refused / sizeof refused[0]; i++) {
      st_options o = { -1.0, 0, 0, 0, refused[i] };
      CHECK(st_solve_device_half(NULL, c, dummy, 4, (float*)dummy, NULL, &lam, &it, &o,
                                 NULL) < 0 && says("not supported"));
      CHECK(max_eigen_value_half_ex(NULL, c, dummy, &lam, v, 4, &it, &o, NULL) < 0 &&
            says("not supported"));
    }
    /* accepted flags reach the queue check */
    st_options ok = { 0.0, 7, ST_SEM_MAINPY, 3, ST_FLAG_MATRIX_FREE | ST_FLAG_TIME_KERNELS |
                                                 ST_FLAG_TRACE_SUMS };
    CHECK(st_solve_device_half(NULL, c, dummy, 4, (float*)dummy, NULL, &lam, &it, &ok,
                               NULL) < 0 && says("null queue"));
    CHECK(max_eigen_value_half_ex(NULL, c, dummy, &lam, v, 4, &it, &ok, NULL) < 0 &&
          says("null queue"));
    st_options sem = { -1.0, 0, 9, 0, 0 };
    CHECK(st_solve_device_half(dummy, c, dummy, 4, (float*)dummy, NULL, &lam, &it, &sem,
                               NULL) < 0 && says("semantics"));
    CHECK(st_solve_device_half(NULL, c, (void*)4097, 4, (float*)dummy, NULL, &lam, &it, NULL,
                               NULL) < 0 && says("aligned"));

    /* step calls */
    CHECK(st_rowsum_half(c, NULL, (float*)dummy, 4, 4, NULL) < 0 && says("null"));
    CHECK(st_rowsum_half(c, dummy, NULL, 4, 4, NULL) < 0 && says("null"));
    CHECK(st_rowsum_half(c, (void*)4097, (float*)dummy, 4, 4, NULL) < 0 && says("aligned"));
    CHECK(st_rowsum_half(c, dummy, (float*)dummy, 0, 4, NULL) == 0);
    CHECK(st_rowsum_half(c, dummy, (float*)dummy, 4, 0, NULL) < 0);
    CHECK(st_narrow_f32(c, NULL, NULL, 0, NULL) == 0);
    CHECK(st_narrow_f32(c, NULL, dummy, 8, NULL) < 0 && says("null"));
    CHECK(st_mfree_round_half(c, NULL, (float*)dummy, (float*)dummy, (float*)dummy,
                              (float*)dummy2, 4, 4, 0, 1e-3f, 1, 10, 0, st, NULL) < 0 &&
          says("null"));
    CHECK(st_mfree_round_half(c, dummy, (float*)dummy, (float*)dummy, (float*)dummy,
                              (float*)dummy2, 4, 4, 0, 1e-3f, 1, 10, 0, NULL, NULL) < 0 &&
          says("null"));
    CHECK(st_mfree_round_half(c, (void*)4099, (float*)dummy, (float*)dummy, (float*)dummy,
                              (float*)dummy2, 4, 4, 0, 1e-3f, 1, 10, 0, st, NULL) < 0 &&
          says("aligned"));
    CHECK(st_mfree_round_half(c, dummy, (float*)dummy, (float*)dummy, (float*)dummy,
                              (float*)dummy2, 0, 4, 0, 1e-3f, 1, 10, 0, st, NULL) < 0 &&
          says("empty"));
    CHECK(st_mfree_round_half(c, dummy, (float*)dummy, (float*)dummy, (float*)dummy,
                              (float*)dummy2, 4, 4, 0, 1e-3f, 0, 10, 0, st, NULL) < 0 &&
          says("k must be >= 1"));
    CHECK(st_mfree_round_half(c, dummy, (float*)dummy, (float*)dummy, (float*)dummy,
                              (float*)dummy2, 4, 4, 0, 1e-3f, 1, 0, 0, st, NULL) < 0);
    CHECK(st_mfree_round_half(c, dummy, (float*)dummy, (float*)dummy, (float*)dummy,
                              (float*)dummy2, 4, 4, 0, 1e-3f, 1, 10, 2, st, NULL) < 0 &&
          says("semantics"));
    CHECK(st_mfree_round_half(c, dummy, (float*)dummy, (float*)dummy, (float*)dummy,
                              (float*)dummy, 4, 4, 0, 1e-3f, 1, 10, 0, st, NULL) < 0 &&
          says("differ"));
    /* rows past the columns, the sum taken in 64 bits */
    CHECK(st_mfree_round_half(c, dummy, (float*)dummy, (float*)dummy, (float*)dummy,
                              (float*)dummy2, 4, 4, 1, 1e-3f, 1, 10, 0, st, NULL) < 0 &&
          says("exceed"));
    CHECK(st_mfree_round_half(c, dummy, (float*)dummy, (float*)dummy, (float*)dummy,
                              (float*)dummy2, 2, 0xffffffffu, 0xffffffffu, 1e-3f, 1, 10, 0, st,
                              NULL) < 0 && says("exceed"));
  }
  /* the dtype parameters of the other calls keep knowing 0 and 1 only */
  CHECK(max_eigen_value_ex(dummy, ST_STORE_F16, dummy, &lam, v, 4, &it, NULL, NULL) < 0 &&
        says("dtype must be 0"));
  CHECK(st_solve_batched_max_dim(ST_STORE_BF16) == 0);
  CHECK(strncmp(st_half_shape_desc(), "rows=", 5) == 0);

  /* with a device: one small host-pointer solve per format (integers 1 .. 8,
     exact in both), against the fp32 solve of the same numbers */
  void* wq = NULL;
  make_queue(&wq);
  if (wq) {
    enum { N = 12 };
    uint16_t h[2][N * N];
    float w[N * N], vh[N], vw[N], lw = 0;
    unsigned int itw = 0;
    for (int i = 0; i < N * N; i++) {
      const int x = 1 + (i * 7 + i / N) % 8;
      h[0][i] = f16_of(x);
      h[1][i] = bf16_of(x);
      w[i] = (float)x;
    }
    st_options mf = { -1.0, 0, 0, 0, ST_FLAG_MATRIX_FREE };
    CHECK(max_eigen_value_ex(wq, 0, w, &lw, vw, N, &itw, &mf, NULL) >= 0);
    for (int c = ST_STORE_F16; c <= ST_STORE_BF16; c++) {
      CHECK(max_eigen_value_half_ex(wq, c, h[c - ST_STORE_F16], &lam, vh, N, &it, NULL,
                                    NULL) >= 0);
      CHECK(it == itw && lam > 0 && (lam - lw) * (lam - lw) <= 1e-10f * lw * lw);
    }
    destroy_queue(wq);
    printf("device paths run\n");
  }
  if (fails) {
    fprintf(stderr, "%d checks failed\n", fails);
    return 1;
  }
  printf("half C-ABI host code clean under ASan/UBSan\n");
  return 0;
}
