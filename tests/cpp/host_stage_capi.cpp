// Test-only C wrapper around the layout layer of elfi_amd/csrc/host_stage.hpp (tests/test_host_stage.py): plain C++, no HIP.
// With -DHOST_STAGE_MAIN it is a program that runs the test's cases itself, for a sanitizer build.
#include "../../elfi_amd/csrc/host_stage.hpp"

using namespace elfihip;

extern "C" {

unsigned long long hs_align(void) { return STAGE_ALIGN; }

// nb blocks of elem[i] x count[i] bytes, present[i] != 0; offsets[i] receives a present block's offset (an absent block's
// entry stays as it was) and *total the bytes needed.  Returns 1, or 0 when the sizes overflow size_t.
int hs_layout(int nb, const unsigned long long* elem, const unsigned long long* count, const int* present,
              unsigned long long* offsets, unsigned long long* total) {
  StageBlock b[16];
  if (nb > 16) return -1;
  for (int i = 0; i < nb; ++i) b[i] = StageBlock{(size_t)elem[i], (size_t)count[i], present[i] != 0, 0};
  size_t t = 0;
  if (!stage_layout(b, nb, &t)) return 0;
  for (int i = 0; i < nb; ++i)
    if (b[i].present) offsets[i] = b[i].offset;
  *total = t;
  return 1;
}

}  // extern "C"

#ifdef HOST_STAGE_MAIN
#include <cstdio>

static int failures = 0;

static void expect(const char* what, int nb, const unsigned long long* elem, const unsigned long long* count, const int* present,
                   int want_ok, const unsigned long long* want_off, unsigned long long want_total) {
  unsigned long long off[16], total = 0;
  for (int i = 0; i < 16; ++i) off[i] = ~0ull;
  const int ok = hs_layout(nb, elem, count, present, off, &total);
  bool good = ok == want_ok;
  for (int i = 0; good && want_ok && i < nb; ++i) good = off[i] == (present[i] ? want_off[i] : ~0ull);
  if (good && want_ok) good = total == want_total;
  if (!good) ++failures;
  printf("%-28s %s\n", what, good ? "ok" : "FAILED");
}

int main() {
  const unsigned long long A = ~0ull;   // an absent block's offset
  const unsigned long long elem[4] = {8, 4, 8, 1}, count[4] = {3, 3, 5, 7};
  {
    const int p[4] = {1, 1, 1, 1};
    const unsigned long long off[4] = {0, 64, 128, 192};
    expect("every block present", 4, elem, count, p, 1, off, 199);
  }
  {
    const int p[4] = {0, 0, 0, 0};
    const unsigned long long off[4] = {A, A, A, A};
    expect("every block absent", 4, elem, count, p, 1, off, 0);
  }
  for (int gone = 0; gone < 4; ++gone) {
    int p[4] = {1, 1, 1, 1};
    p[gone] = 0;
    unsigned long long off[4] = {A, A, A, A}, at = 0, end = 0;
    for (int i = 0; i < 4; ++i) {
      if (!p[i]) continue;
      off[i] = at;
      end = at + elem[i] * count[i];
      at += 64;   // every block here is shorter than 64 bytes
    }
    expect("one block absent", 4, elem, count, p, 1, off, end);
  }
  {
    const unsigned long long e[3] = {4, 8, 1}, c[3] = {3, 1, 65}, off[3] = {0, 64, 128};
    const int p[3] = {1, 1, 1};
    expect("int32 x 3 before int64", 3, e, c, p, 1, off, 193);
  }
  {
    const unsigned long long e[3] = {8, 4, 8}, c[3] = {2, 0, 2}, off[3] = {0, 64, 64};
    const int p[3] = {1, 1, 1};
    expect("a zero count", 3, e, c, p, 1, off, 80);
  }
  {
    const unsigned long long e[2] = {8, 8}, c[2] = {1, ~0ull / 8}, off[2] = {0, 0};
    const int p[2] = {1, 1};
    expect("sum overflows", 2, e, c, p, 0, off, 0);
    const unsigned long long e1[1] = {8}, c1[1] = {~0ull / 8 + 1};
    expect("product overflows", 1, e1, c1, p, 0, off, 0);
    const unsigned long long e2[2] = {1, 1}, c2[2] = {~0ull - 10, 1};
    expect("alignment overflows", 2, e2, c2, p, 0, off, 0);
  }
  printf("%d failure(s)\n", failures);
  return failures != 0;
}
#endif
