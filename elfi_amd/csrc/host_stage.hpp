// How the host-pointer forms of the example simulators and their samplers (series.hip, gnk.hip, lorenz.hip, toad.hip, sv.hip,
// gillespie.hip, daycare.hip, scratch_assay.hip, bdm.hip, poisson.hip, stable.hip, stable_general.hip) stage their arrays:
// the layout of the blocks of one buffer -- plain C++, no HIP, no context: tests/test_host_stage.py checks it without a GPU --
// and, for hipcc, the staging of a call's arrays through the context's `in` and `out` buffers.
#pragma once

#include <cstddef>
#include <cstdint>

namespace elfihip {

constexpr size_t STAGE_ALIGN = 64;   // every present block starts at a multiple of this: the order of the blocks is free

struct StageBlock {
  size_t elem, count;   // bytes per element, elements
  bool present;         // an absent block takes no room
  size_t offset;        // set by stage_layout for a present block: where it starts, in bytes
};

// Lays the present blocks out one behind the other; *total receives the bytes they need.  false: the sizes overflow size_t.
inline bool stage_layout(StageBlock* b, int nb, size_t* total) {
  size_t end = 0;
  for (int i = 0; i < nb; ++i) {
    if (!b[i].present) continue;
    if (end > SIZE_MAX - (STAGE_ALIGN - 1)) return false;
    const size_t at = (end + STAGE_ALIGN - 1) / STAGE_ALIGN * STAGE_ALIGN;
    if (b[i].count != 0 && b[i].elem > (SIZE_MAX - at) / b[i].count) return false;
    b[i].offset = at;
    end = at + b[i].elem * b[i].count;
  }
  *total = end;
  return true;
}

}  // namespace elfihip

#if defined(__HIPCC__)
#include "common.hpp"

namespace elfihip {

// The arrays of ONE host-form call.  Between upload() and download() it owns ctx->in and ctx->out: the _dev implementation
// called in between borrows neither (ctx->par, ctx->sim and the work buffers are theirs).  Nothing is kept in the context:
// DevBuf::reserve may move a buffer at the next call.  An array whose host pointer is NULL is absent: no room, no copy, and
// its device slot is NULL -- what the _dev implementation takes as "not given" / "not asked for".
class HostStage {
 public:
  explicit HostStage(elfihip_ctx* ctx) : ctx_(ctx) {}
  template <class T>
  void in(T** slot, const T* host, size_t count) { add(0, slot, const_cast<T*>(host), sizeof(T), count); }
  template <class T>
  void out(T** slot, T* host, size_t count) { add(1, slot, host, sizeof(T), count); }

  // Reserves `in` and `out` once each, fills the slots and enqueues the inputs' copies on the stream, in the order given.
  int upload() {
    DevBuf* buf[2] = {&ctx_->in, &ctx_->out};
    for (int s = 0; s < 2; ++s) {
      size_t total = 0;
      if (n_[s] > CAP || !stage_layout(blk_[s], n_[s], &total))
        return fail(ctx_, ELFIHIP_ERR_NOMEM, "the arrays of this call do not fit a staging buffer");
      ELFIHIP_CHECK_HIP(ctx_, buf[s]->reserve(total));
      for (int i = 0; i < n_[s]; ++i) {
        void* d = blk_[s][i].present ? buf[s]->as<char>() + blk_[s][i].offset : nullptr;
        memcpy(slot_[s][i], &d, sizeof d);
      }
    }
    return copy(0);
  }
  // After the launches: enqueues the outputs' copies, in the order given, and waits for the stream.
  int download() {
    ELFIHIP_TRY(copy(1));
    ELFIHIP_CHECK_HIP(ctx_, hipStreamSynchronize(ctx_->stream));
    return ELFIHIP_OK;
  }

 private:
  static constexpr int CAP = 12;   // arrays per direction (sv.hip: eleven inputs)
  void add(int s, void* slot, void* host, size_t elem, size_t count) {
    if (n_[s] < CAP) {
      blk_[s][n_[s]] = StageBlock{elem, count, host != nullptr, 0};
      slot_[s][n_[s]] = slot;
      host_[s][n_[s]] = host;
    }
    ++n_[s];
  }
  int copy(int s) {
    const char* base = (s ? ctx_->out : ctx_->in).as<char>();
    for (int i = 0; i < n_[s]; ++i) {
      const StageBlock& b = blk_[s][i];
      if (!b.present) continue;
      void* d = const_cast<char*>(base) + b.offset;
      ELFIHIP_CHECK_HIP(ctx_, hipMemcpyAsync(s ? host_[s][i] : d, s ? d : host_[s][i], b.elem * b.count,
                                             s ? hipMemcpyDeviceToHost : hipMemcpyHostToDevice, ctx_->stream));
    }
    return ELFIHIP_OK;
  }
  elfihip_ctx* ctx_;
  StageBlock blk_[2][CAP];
  void* slot_[2][CAP];   // where each array's device pointer goes (a T**)
  void* host_[2][CAP];
  int n_[2] = {0, 0};
};

}  // namespace elfihip
#endif
