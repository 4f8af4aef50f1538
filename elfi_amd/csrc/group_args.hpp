// What the group-statistic entry points (synlik.hip, semibsl.hip, logratio.hip: one workgroup per group of summary rows,
// m <= 64 columns in tiles of 16) settle on the host: the check of the prefix and penalty lists, the parameter block the
// kernels read them from, the tile count.  No HIP, no context: tests/test_group_args.py checks them without a GPU.
#pragma once

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

namespace elfihip {

// 16-column tiles that hold m columns
inline int group_tiles(int m) { return (m + 15) / 16; }

// The lists of a call over n rows per group: K prefixes (or none: the whole group) and P penalties (or none).  Returns what
// is wrong with them, in the words the caller reports, or an empty string.  (A NaN penalty fails both comparisons.)
inline std::string group_lists_error(const int64_t* prefixes, int K, const double* penalties, int P, int64_t n) {
  char buf[96];
  const auto text = [&](const char* fmt, int v) {
    snprintf(buf, sizeof buf, fmt, v);
    return std::string(buf);
  };
  if (!((prefixes && K >= 1) || (!prefixes && K <= 1))) return text("prefixes and K do not agree (K=%d)", K);
  if (!((penalties && P >= 1) || (!penalties && P == 0))) return text("penalties and P do not agree (P=%d)", P);
  if (prefixes) {
    for (int k = 0; k < K; ++k)
      if (!(prefixes[k] >= 2 && (k == 0 || prefixes[k] > prefixes[k - 1])))
        return text("prefixes must be ascending and at least 2 (entry %d)", k);
    if (prefixes[K - 1] != n) return "the last prefix must be n";
  }
  for (int p = 0; p < P; ++p)
    if (!(penalties[p] >= 0.0 && penalties[p] <= 1.0)) return text("penalty %d is outside [0, 1]", p);
  return std::string();
}

// The parameter block of checked lists: [Ke prefixes as int64 bit patterns][Ke constants, only if given][P penalties].
// Ke = K, or 1 without prefixes (the one prefix is n).  konst: one value per prefix, or NULL.
struct GroupParams {
  std::vector<double> words;
  int Ke;
  size_t konst, pen;   // where the constants and the penalties begin, in doubles
};

inline GroupParams group_params(const int64_t* prefixes, int K, int64_t n, const double* konst, const double* penalties,
                                int P) {
  GroupParams B;
  B.Ke = prefixes ? K : 1;
  B.konst = (size_t)B.Ke;
  B.pen = (size_t)B.Ke * (konst ? 2 : 1);
  B.words.resize(B.pen + (size_t)P);
  for (int k = 0; k < B.Ke; ++k) {
    const int64_t p = prefixes ? prefixes[k] : n;
    memcpy(&B.words[k], &p, sizeof p);
    if (konst) B.words[B.konst + k] = konst[k];
  }
  for (int p = 0; p < P; ++p) B.words[B.pen + p] = penalties[p];
  return B;
}

}  // namespace elfihip
