// stream_pipe.h — the lanes of host_pipeline.h's chunk loop on the device: two copy streams beside the context's stream, and
// one event per stage and chunk.
#pragma once

#include "common.h"
#include "host_pipeline.h"

namespace earhip {

// Copy streams and events of long host-pointer calls (made at the first such call and kept): the chunks of a call go
// H2D on `in`, through the kernels on `stream` (the context's, set for the duration of a call), and D2H on `out`, each stage
// ordered behind the one before it by the chunk's events — chunk c's kernels and the transfer of its outputs run beside the
// transfer of c + 1.  The six operations run_host_chunks asks of its lanes; Status is HIP's (hipSuccess == hipError_t()).
struct StreamPipe {
  hipStream_t in = nullptr, out = nullptr, stream = nullptr;
  hipEvent_t ev_in[GatherPool::kMaxGroups] = {}, ev_k[GatherPool::kMaxGroups] = {}, ev_out[GatherPool::kMaxGroups] = {};
  bool made = false;
  void make() {
    if (made) return;
    try {
      EARHIP_HIP(hipStreamCreateWithFlags(&in, hipStreamNonBlocking));
      EARHIP_HIP(hipStreamCreateWithFlags(&out, hipStreamNonBlocking));
      for (int i = 0; i < GatherPool::kMaxGroups; i++) {
        EARHIP_HIP(hipEventCreateWithFlags(&ev_in[i], hipEventDisableTiming));
        EARHIP_HIP(hipEventCreateWithFlags(&ev_k[i], hipEventDisableTiming));
        EARHIP_HIP(hipEventCreateWithFlags(&ev_out[i], hipEventDisableTiming));
      }
    } catch (...) {
      destroy();  // (what the creates before the failing one made)
      throw;
    }
    made = true;
  }
  void destroy() {
    for (int i = 0; i < GatherPool::kMaxGroups; i++)
      for (hipEvent_t *e : {&ev_in[i], &ev_k[i], &ev_out[i]}) {
        if (*e) (void)hipEventDestroy(*e);
        *e = nullptr;
      }
    for (hipStream_t *s : {&in, &out}) {
      if (*s) (void)hipStreamDestroy(*s);
      *s = nullptr;
    }
    made = false;
  }
  ~StreamPipe() { destroy(); }
  // at the head of a long call: streams and events made at the first one, the context's stream taken for this one
  void begin(hipStream_t compute) {
    make();
    stream = compute;
  }

  hipError_t in_done(int c) {
    const hipError_t e = hipEventRecord(ev_in[c], in);
    return e != hipSuccess ? e : hipStreamWaitEvent(stream, ev_in[c], 0);
  }
  hipError_t kernels_done(int c) {
    const hipError_t e = hipEventRecord(ev_k[c], stream);
    return e != hipSuccess ? e : hipStreamWaitEvent(out, ev_k[c], 0);
  }
  hipError_t out_done(int c) { return hipEventRecord(ev_out[c], out); }
  bool out_landed(int c) { return hipEventQuery(ev_out[c]) == hipSuccess; }
  void drain() {
    (void)hipStreamSynchronize(in);
    (void)hipStreamSynchronize(stream);
    (void)hipStreamSynchronize(out);
  }
  void raise(hipError_t err) { EARHIP_HIP(err); }
};

}  // namespace earhip
