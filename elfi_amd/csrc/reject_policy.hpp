// What happens to a batch when it meets the sampler state (reject.hip): thresholds, route, merge cadence and sizes as plain
// functions of a few numbers -- no HIP, no state object -- for every push form; tests/test_reject_policy.py checks them.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>

namespace elfihip {

constexpr int REJ_MERGE_EVERY = 8;                 // pushes per merge, at most
constexpr unsigned int REJ_CAP = 1u << 16;         // smallest candidate list
constexpr double REJ_HEAVY = 8192.0;               // expected candidates from which a push takes the radix selection
constexpr int64_t REJ_ACC_SELECT_MIN = 1 << 15;    // batch rows from which an acceptance push selects instead of listing
constexpr int64_t REJ_PROV_MIN_ROWS = 1 << 20;     // batch rows from which a first batch takes a provisional threshold
constexpr unsigned int REJ_PROV_MAX_CAND = 1u << 16;   // ... and the candidates it may then list

// The state as a push meets it.  entered: rows it holds (host-merge states: in the host copy); rows_seen: BEFORE this push.
struct RejMeet {
  int64_t k, entered, rows_seen;
  bool host_mode, has_accept;
  bool full() const { return entered >= k; }
};

enum class RejRoute {
  AcceptSelect,   // mask the rows outside the acceptance thresholds, count, radix selection of the k best, merge
  Select,         // plain pass, radix selection of the batch's k best, merge
  Provisional,    // a large first batch: threshold from a prefix of the batch, the rest filtered against it
  Filter,         // the rows below the state's k-th distance go to the candidate list
};

// n rows arrive.  can_prefix: the caller's pass can run over a prefix of the batch and then over the rest.
inline RejRoute rej_route(const RejMeet& S, int64_t n, bool can_prefix) {
  // rows this push is expected to offer against the current threshold (batches of one distribution): n k / rows seen
  const double expect = S.full() ? (double)n * (double)S.k / (double)std::max<int64_t>(S.rows_seen, 1) : 1e300;
  const bool heavy = expect > REJ_HEAVY;   // every row could enter (still filling up) or very many would: no list
  if (S.has_accept) return !S.host_mode && n >= REJ_ACC_SELECT_MIN && heavy ? RejRoute::AcceptSelect : RejRoute::Filter;
  if (!heavy) return RejRoute::Filter;
  return can_prefix && !S.full() && n >= REJ_PROV_MIN_ROWS && 64 * S.k <= n ? RejRoute::Provisional : RejRoute::Select;
}

// Filtered pushes between two merges.  The p-th push after the state became full offers about k / p candidates (batches of
// one distribution), so merging every p / 2 pushes -- at most every REJ_MERGE_EVERY-th -- keeps a merge at about k / 2
// candidates: early on, while the threshold still falls quickly, after every push.  A state that seals its lists (the merge
// rides on the next row pass) seals every p / 3 pushes instead: about k / 3 candidates, which one wave sorts and merges
// inside the pass (measured at 10^6 x 32, k = 1000: lists of <= 512 cost the pass 1-2 us; lists just above 512 -- the
// 1024-entry sort -- 25 us more than the pass).  Host-merge states and states that are still filling merge after every push.
inline int64_t rej_merge_interval(int64_t armed_pushes, bool seals, bool host_mode, bool full) {
  if (host_mode || !full) return 1;
  return std::min<int64_t>(std::max<int64_t>(armed_pushes / (seals ? 3 : 2), 1), REJ_MERGE_EVERY);
}

// Provisional route: a prefix of s rows; its j-th smallest distance is the threshold for the rest (j: five standard
// deviations above the k s / n of the batch's k best that fall into a prefix of exchangeable rows); a list of k .. c_hi
// candidates shows that the prefix represented the batch.  (s = n / 16: j n / s = 1700 +- 160 candidates for k = 1000,
// two 1024-chunks of the merge; with n / 32 they were 2050 +- 250, a third chunk every other round.)
struct RejProv { int64_t s, j, c_hi; };
inline RejProv rej_provisional(int64_t n, int64_t k, int64_t cap) {
  RejProv P;
  P.s = std::min<int64_t>(std::max<int64_t>(n / 16, 16384), n / 2);
  const double mu = (double)k * (double)P.s / (double)n;
  P.j = std::min<int64_t>(k, (int64_t)std::ceil(mu + 5.0 * std::sqrt(mu) + 4.0));
  P.c_hi = std::min<int64_t>(std::max<int64_t>(REJ_PROV_MAX_CAND, 64 * P.j), cap);
  return P;
}

// Entries of a candidate list for batches of n rows: it receives at most REJ_MERGE_EVERY pushes before it is merged or sealed.
inline int64_t rej_list_size(int64_t n) { return std::max<int64_t>(REJ_CAP, REJ_MERGE_EVERY * n); }

}  // namespace elfihip
