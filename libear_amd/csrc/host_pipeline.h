// host_pipeline.h — the chunked pipeline of long calls from host memory (earhip_render_process, _process_frames and _frames_pcm:
// api_render.hip): the staging threads and the ONE loop that runs a call's time chunks through three lanes of the device; a
// chunk's transfers and kernels are the caller's callables, the lanes a type of the caller's (the copy streams and events:
// stream_pipe.h).  The plan and the copies the threads make: host_gather.h.  Plain C++17 and threads, no device interface: a
// stand-alone program drives this pool and this loop against lanes made of threads, under the thread and address sanitizers
// (tests/cpp/test_host_pipeline.cpp).
#pragma once

#include <atomic>
#include <condition_variable>
#include <exception>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "errors.h"
#include "host_gather.h"

namespace earhip {

// Staging threads of the host-pointer entry point, started at the first long call and kept: a call
// neither creates threads nor allocates.  A long call is cut into TIME chunks (a few blocks each: ~8 MB of inputs); a job =
// gather every channel's samples of chunk g into the pinned buffer, chunk-major ([chunk][channel][samples of the chunk]: a
// chunk is one linear transfer), thread t taking every nthreads-th channel; done[g] counts the threads that have finished
// chunk g (the caller starts that chunk's transfer then, while the threads gather the next one).  The contiguous-range job
// (submit_range: interleaved PCM frames, earhip_render_process_frames) copies chunk g's byte range of the caller's buffer to the
// same offset of the pinned buffer instead, thread t taking its slice of the range (range_slice).
struct GatherPool {
  static constexpr int kMaxGroups = HostChunkPlan::kMaxChunks;
  NumaMap numa;
  bool streaming = true;              // (option HOST_NT, read when a job is submitted)
  int job_node = -1;                  // the node this job's rows live on (-1: run anywhere)
  const cpu_set_t *job_cpus = nullptr;
  std::vector<std::thread> threads;
  std::mutex mu;
  std::condition_variable go, finished_cv;
  uint64_t generation = 0;
  int finished = 0;
  bool quit = false;
  // the job
  const float *const *in = nullptr;
  float *dst = nullptr;
  size_t n = 0;                      // samples per channel in the call
  size_t cstart[kMaxGroups + 1] = {0};  // chunk g = samples [cstart[g], cstart[g + 1]) of every channel
  int M = 0, groups = 0;
  const unsigned char *src_bytes = nullptr;  // contiguous-range job: source and destination of chunk g = bytes
  unsigned char *dst_bytes = nullptr;        // [cstart[g] * unit, cstart[g + 1] * unit) (src_bytes NULL: a row job)
  size_t unit = 0;
  std::atomic<int> done[kMaxGroups];
  int nthreads() const { return (int)threads.size(); }
  size_t group_len(int g) const { return cstart[g + 1] - cstart[g]; }
  void start(int count) {
    for (int t = 0; t < count; t++)
      threads.emplace_back([this, t] {
        uint64_t seen = 0;
        int my_node = -1;  // the node this thread is bound to (-1: not bound)
        for (;;) {
          int want_node;
          const cpu_set_t *want_cpus;
          {
            std::unique_lock<std::mutex> lk(mu);
            go.wait(lk, [&] { return quit || generation != seen; });
            if (quit) return;
            seen = generation;
            want_node = job_node, want_cpus = job_cpus;
          }
          if (want_node != my_node) {  // (a failure leaves the thread where it is: placement is an optimisation)
            if (want_node >= 0 && want_cpus) {
              if (sched_setaffinity(0, sizeof(cpu_set_t), want_cpus) == 0) my_node = want_node;
            } else if (numa.ok && sched_setaffinity(0, sizeof(cpu_set_t), &numa.allowed) == 0) {
              my_node = -1;
            }
          }
          const int nt = nthreads();
          for (int g = 0; g < groups; g++) {
            const size_t len = group_len(g), at = cstart[g];
            float *base = dst + (size_t)M * at;
            if (src_bytes) {
              size_t lo, hi;
              range_slice(len * unit, t, nt, &lo, &hi);
              const size_t o = at * unit + lo;
              if (hi > lo) {
                if (streaming) stream_copy_bytes(dst_bytes + o, src_bytes + o, hi - lo);
                else std::memcpy(dst_bytes + o, src_bytes + o, hi - lo);
              }
            } else if (streaming) {
              for (int m = t; m < M; m += nt) stream_copy(base + (size_t)m * len, in[m] + at, len);
            } else {
              for (int m = t; m < M; m += nt) std::memcpy(base + (size_t)m * len, in[m] + at, sizeof(float) * len);
            }
#if defined(__x86_64__)
            if (streaming) _mm_sfence();  // (streaming stores are weakly ordered: globally visible before the chunk counts as gathered)
#endif
            done[g].fetch_add(1, std::memory_order_release);
          }
          std::lock_guard<std::mutex> lk(mu);
          if (++finished == nt) finished_cv.notify_one();
        }
      });
  }
  // (under mu) the part of a job both kinds share: its chunks, where its threads run, and the go
  void publish(const size_t *starts, int nchunks, int node, bool nt) {
    for (int g = 0; g <= nchunks; g++) cstart[g] = starts[g];
    streaming = nt;
    job_cpus = numa.cpus_of(node);
    job_node = job_cpus ? node : -1;
    groups = nchunks;
    for (auto &d : done) d.store(0);
    finished = 0;
    generation++;
    go.notify_all();
  }
  void submit(const float *const *in_, float *dst_, size_t n_, const size_t *starts, int nchunks, int M_, bool bind, bool nt) {
    const int node = bind && numa.ok ? NumaMap::rows_node(in_, M_, n_) : -1;
    std::lock_guard<std::mutex> lk(mu);
    in = in_, dst = dst_, n = n_, M = M_;
    src_bytes = nullptr;
    publish(starts, nchunks, node, nt);
  }
  void submit_range(const void *src, void *dst_, size_t unit_, const size_t *starts, int nchunks, bool bind, bool nt) {
    const int node = bind && numa.ok ? NumaMap::range_node(src, starts[nchunks] * unit_) : -1;
    std::lock_guard<std::mutex> lk(mu);
    src_bytes = static_cast<const unsigned char *>(src), dst_bytes = static_cast<unsigned char *>(dst_), unit = unit_;
    in = nullptr, dst = nullptr, n = starts[nchunks], M = 0;
    publish(starts, nchunks, node, nt);
  }
  void wait_all() {
    std::unique_lock<std::mutex> lk(mu);
    finished_cv.wait(lk, [&] { return finished == nthreads(); });
  }
  ~GatherPool() {
    {
      std::lock_guard<std::mutex> lk(mu);
      quit = true;
    }
    go.notify_all();
    for (auto &th : threads) th.join();
  }
};

struct HostChunkTimes { double enqueued = 0.0, drained = 0.0; };  // the last chunk enqueued, the gather through / all of it drained

// The chunks of `plan` — chunk c = samples [at, at + len) of every channel — through three stages on three lanes of the device,
// each a queue that runs what it is given in order: the transfer in of chunk c + 1 (the in lane) beside the kernels of chunk c (the
// compute lane) beside the transfer out of chunk c - 1 (the out lane), one mark per stage and chunk.  `lanes` orders them, and is
// all this loop knows of the device (StreamPipe, stream_pipe.h: streams and events; the CPU test: threads):
//   Status in_done(c)       chunk c's input transfer is queued: mark it on the in lane, and the compute lane waits for the mark
//   Status kernels_done(c)  mark on the compute lane, and the out lane waits for it
//   Status out_done(c)      mark on the out lane
//   bool out_landed(c)      has the mark of out_done(c) been reached (never blocks; a mark keeps its state from call to call)
//   void drain()            waits for the in, compute and out lanes, in that order; never throws
//   void raise(Status)      throws Error for a status that is not success
// Status is the lanes' own type, a default-constructed one means success.  gather: the staging threads, their job submitted (a
// chunk is enqueued once they have gathered it), or nullptr.  h2d / d2h (at, len) enqueue a chunk's transfer on the in / out lane
// and return a Status; kernels(at, len) enqueues on the compute lane and may throw.  staged_out: outputs return through pinned
// staging and scatter(at, len) hands a landed chunk to the caller, while the call waits for the gather and at the end — only chunks
// whose output transfer THIS call marked (a mark of an earlier call says nothing about this one), and none once anything has failed.
// NO EXCEPTION LEAVES A CALL MID-FLIGHT: whatever kernels throws is caught here, and after that, or after a Status that is not
// success, nothing more is enqueued, the staging threads still finish their job and the lanes are drained; only then is the first
// bad Status raised, or Error{EARHIP_INTERNAL_ERROR, the message thrown} (an Error's msg, a std::exception's what(); out of memory
// reads as it does at the C boundary).  When the call returns or throws, nothing reads or writes the caller's or the staging buffers.
// now(): the caller's clock for the two times returned; *chunks_run = the number of chunks, on success.
template <typename Lanes, typename H2D, typename Kernels, typename D2H, typename Scatter, typename Clock>
HostChunkTimes run_host_chunks(Lanes &lanes, GatherPool *gather, const HostChunkPlan &plan, bool staged_out, int *chunks_run, H2D h2d,
                               Kernels kernels, D2H d2h, Scatter scatter, Clock now) {
  using Status = decltype(lanes.in_done(0));
  const int nch = plan.nch;
  const size_t *at = plan.cstart;
  const auto len = [at](int c) { return at[c + 1] - at[c]; };
  Status err = Status();
  bool thrown = false;
  std::string fail;
  const auto ok = [&] { return err == Status() && !thrown; };
  int recorded = 0;   // chunks whose output transfer this call has queued and marked
  int scattered = 0;  // ... whose outputs have been handed to the caller
  for (int c = 0; c < nch; c++) {
    if (gather) {
      while (gather->done[c].load(std::memory_order_acquire) < gather->nthreads()) {
        if (staged_out && scattered < recorded && ok() && lanes.out_landed(scattered))
          scatter(at[scattered], len(scattered)), scattered++;
        else
          std::this_thread::yield();
      }
    }
    if (!ok()) continue;  // (the staging threads still finish their job)
    err = h2d(at[c], len(c));
    if (ok()) err = lanes.in_done(c);
    if (!ok()) continue;
    try {
      kernels(at[c], len(c));
    } catch (const Error &e) {
      thrown = true, fail = e.msg;
    } catch (const std::bad_alloc &) {
      thrown = true, fail = "out of host memory";
    } catch (const std::exception &e) {
      thrown = true, fail = e.what();
    } catch (...) {
      thrown = true, fail = "unknown exception";
    }
    if (ok()) err = lanes.kernels_done(c);
    if (ok()) err = d2h(at[c], len(c));
    if (ok()) err = lanes.out_done(c);
    if (ok()) recorded = c + 1;
  }
  if (gather) gather->wait_all();
  HostChunkTimes times;
  times.enqueued = now();
  lanes.drain();  // (whatever happened above: nothing of this call is in flight when it returns)
  lanes.raise(err);
  if (thrown) throw Error{EARHIP_INTERNAL_ERROR, fail};
  times.drained = now();
  if (staged_out)
    for (; scattered < nch; scattered++) scatter(at[scattered], len(scattered));
  *chunks_run = nch;
  return times;
}

}  // namespace earhip
