// Test-only C wrapper around elfi_amd/csrc/reject_policy.hpp (tests/test_reject_policy.py): plain C++, no HIP.
#include "../../elfi_amd/csrc/reject_policy.hpp"

using namespace elfihip;

extern "C" {

// 0: accept-and-select, 1: select, 2: provisional, 3: filter
int rp_route(long long k, long long entered, long long rows_seen, int host_mode, int has_accept, long long n, int can_prefix) {
  const RejMeet S{k, entered, rows_seen, host_mode != 0, has_accept != 0};
  switch (rej_route(S, n, can_prefix != 0)) {
    case RejRoute::AcceptSelect: return 0;
    case RejRoute::Select: return 1;
    case RejRoute::Provisional: return 2;
    case RejRoute::Filter: return 3;
  }
  return -1;
}

long long rp_interval(long long armed_pushes, int seals, int host_mode, int full) {
  return rej_merge_interval(armed_pushes, seals != 0, host_mode != 0, full != 0);
}

void rp_provisional(long long n, long long k, long long cap, long long* out3) {
  const RejProv P = rej_provisional(n, k, cap);
  out3[0] = P.s;
  out3[1] = P.j;
  out3[2] = P.c_hi;
}

long long rp_list_size(long long n) { return rej_list_size(n); }

}  // extern "C"
