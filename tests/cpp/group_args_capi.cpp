// Test-only C wrapper around elfi_amd/csrc/group_args.hpp (tests/test_group_args.py): plain C++, no HIP.
#include "../../elfi_amd/csrc/group_args.hpp"

#include <algorithm>

using namespace elfihip;

extern "C" {

int ga_tiles(int m) { return group_tiles(m); }

// The error text goes to buf (empty: the lists are good); returns its length.
int ga_lists_error(const long long* prefixes, int K, const double* penalties, int P, long long n, char* buf, int cap) {
  const std::string e = group_lists_error(reinterpret_cast<const int64_t*>(prefixes), K, penalties, P, n);
  snprintf(buf, (size_t)cap, "%s", e.c_str());
  return (int)e.size();
}

// The parameter block goes to words (room for cap doubles); out3 receives Ke and the offsets of the constants and of the
// penalties; returns the block's length in doubles.
int ga_params(const long long* prefixes, int K, long long n, const double* konst, const double* penalties, int P,
              double* words, int cap, long long* out3) {
  const GroupParams B = group_params(reinterpret_cast<const int64_t*>(prefixes), K, n, konst, penalties, P);
  out3[0] = B.Ke;
  out3[1] = (long long)B.konst;
  out3[2] = (long long)B.pen;
  memcpy(words, B.words.data(), std::min(B.words.size(), (size_t)cap) * sizeof(double));
  return (int)B.words.size();
}

}  // extern "C"
