// libear_amd/csrc/host_pipeline.h on the CPU: the real staging threads (GatherPool) and the real chunk loop (run_host_chunks)
// against a "device" made of threads and memcpy, built with the thread sanitizer and with the address + undefined-behaviour
// sanitizers (tests/test_host_pipeline_cpu.py).
//
// The device is three lanes (in, compute, out), each a worker thread with a FIFO of tasks.  A mark is a flag under a mutex and
// condition variable: recording it on a lane clears it at once and queues a task that sets it; a lane waits for a mark with a task
// that blocks until it is set.  Like an event of the device a mark keeps its state from call to call (one never recorded counts as
// reached), so a stale out_landed is true.  h2d queues a memcpy from the staging buffer to device memory on the in lane, kernels
// queues a per-row recurrence on the compute lane whose state carries over chunk boundaries (the chunk order shows in every later
// sample), d2h queues a memcpy on the out lane and scatter copies to the caller's rows on the calling thread.  Buffers are laid out
// as in api_render.hip: chunk-major, chunk c = [rows][len] at offset rows * at.  Expected: the recurrence over the whole call in
// one piece on the main thread, compared bit for bit.
#include <atomic>
#include <cstdio>
#include <cstring>
#include <deque>
#include <functional>
#include <memory>
#include <stdexcept>

#include "host_pipeline.h"

using namespace earhip;

static thread_local std::string g_last_error;
namespace earhip {
void set_last_error(const std::string &msg) { g_last_error = msg; }
}  // namespace earhip

static std::atomic<int> g_failed{0};
static std::atomic<int> g_cases{0};
#define CHECK(cond, ...)                     \
  do {                                       \
    if (!(cond)) {                           \
      if (g_failed++ < 20) {                 \
        printf("FAILED %s: ", #cond);        \
        printf(__VA_ARGS__);                 \
        printf("\n");                        \
      }                                      \
    }                                        \
  } while (0)

// ---- the device --------------------------------------------------------------------------------------------------------------
struct Lane {
  std::mutex mu;
  std::condition_variable work, idle_cv;
  std::deque<std::function<void()>> fifo;
  bool busy = false, quit = false;
  long queued = 0, ran = 0;
  std::thread th;
  Lane() : th([this] { run(); }) {}
  ~Lane() {
    {
      std::lock_guard<std::mutex> lk(mu);
      quit = true;
    }
    work.notify_all();
    th.join();
  }
  void run() {
    std::unique_lock<std::mutex> lk(mu);
    for (;;) {
      work.wait(lk, [&] { return quit || !fifo.empty(); });
      if (fifo.empty()) return;
      std::function<void()> task = std::move(fifo.front());
      fifo.pop_front();
      busy = true;
      lk.unlock();
      task();
      lk.lock();
      busy = false, ran++;
      if (fifo.empty()) idle_cv.notify_all();
    }
  }
  void push(std::function<void()> task) {
    {
      std::lock_guard<std::mutex> lk(mu);
      fifo.push_back(std::move(task));
      queued++;
    }
    work.notify_one();
  }
  void sync() {
    std::unique_lock<std::mutex> lk(mu);
    idle_cv.wait(lk, [&] { return fifo.empty() && !busy; });
  }
  bool idle() {
    std::lock_guard<std::mutex> lk(mu);
    return fifo.empty() && !busy && queued == ran;
  }
};

enum Op { H2D, IN_DONE, KERNELS, KERNELS_DONE, D2H, OUT_DONE, DRAIN, SCATTER, NONE };
static const char *const kOpName[] = {"h2d", "in_done", "kernels", "kernels_done", "d2h", "out_done", "drain", "scatter", "none"};
struct Ev {
  Op op;
  int c;
  bool operator==(const Ev &o) const { return op == o.op && c == o.c; }
};
// what a call is made to fail with: at chunk `chunk`, stage `op` returns a failure (KERNELS: throws, an Error or a runtime_error)
struct Inject {
  Op op = NONE;
  int chunk = -1;
  bool std_exception = false;
  bool at(Op o, int c) const { return op == o && chunk == c; }
};
struct Status {
  int code = 0;
  bool operator==(const Status &o) const { return code == o.code; }
};
static const Status kInjected{1234};
static const char *const kInjectedText = "injected status 1234";

// what both kinds of lanes share: the order of calls as the loop made them (all on the calling thread), and the failure to inject
struct LanesBase {
  std::vector<Ev> log;
  Inject inj;
  // a gate the failing step opens: a task of the device that waits at it ends only after that step has failed
  std::mutex gate_mu;
  std::condition_variable gate_cv;
  bool gate_open = true;
  void set_gate(bool open) {
    {
      std::lock_guard<std::mutex> lk(gate_mu);
      gate_open = open;
    }
    gate_cv.notify_all();
  }
  void wait_at_gate() {
    std::unique_lock<std::mutex> lk(gate_mu);
    gate_cv.wait(lk, [&] { return gate_open; });
  }
  Status step(Op op, int c) {
    log.push_back({op, c});
    if (!inj.at(op, c)) return Status();
    set_gate(true);
    return kInjected;
  }
  void raise(Status s) {
    if (!(s == Status())) throw Error{EARHIP_DEVICE_ERROR, "injected status " + std::to_string(s.code)};
  }
};

struct ThreadLanes : LanesBase {
  Lane in, compute, out;
  std::mutex mu;
  std::condition_variable reached_cv;
  bool m_in[GatherPool::kMaxGroups], m_k[GatherPool::kMaxGroups], m_out[GatherPool::kMaxGroups];
  ThreadLanes() {
    for (int c = 0; c < GatherPool::kMaxGroups; c++) m_in[c] = m_k[c] = m_out[c] = true;
  }
  void record(bool *mark, Lane &lane) {
    {
      std::lock_guard<std::mutex> lk(mu);
      *mark = false;
    }
    lane.push([this, mark] {
      {
        std::lock_guard<std::mutex> lk(mu);
        *mark = true;
      }
      reached_cv.notify_all();
    });
  }
  void wait(Lane &lane, bool *mark) {
    lane.push([this, mark] {
      std::unique_lock<std::mutex> lk(mu);
      reached_cv.wait(lk, [&] { return *mark; });
    });
  }
  Status in_done(int c) {
    const Status s = step(IN_DONE, c);
    if (s == Status()) record(&m_in[c], in), wait(compute, &m_in[c]);
    return s;
  }
  Status kernels_done(int c) {
    const Status s = step(KERNELS_DONE, c);
    if (s == Status()) record(&m_k[c], compute), wait(out, &m_k[c]);
    return s;
  }
  Status out_done(int c) {
    const Status s = step(OUT_DONE, c);
    if (s == Status()) record(&m_out[c], out);
    return s;
  }
  bool out_landed(int c) {
    std::lock_guard<std::mutex> lk(mu);
    return m_out[c];
  }
  void drain() {
    log.push_back({DRAIN, 0});
    in.sync(), compute.sync(), out.sync();
  }
  bool idle() { return in.idle() && compute.idle() && out.idle(); }
};

// lanes without a device: they only write down what the loop asks of them
struct RecordingLanes : LanesBase {
  Status in_done(int c) { return step(IN_DONE, c); }
  Status kernels_done(int c) { return step(KERNELS_DONE, c); }
  Status out_done(int c) { return step(OUT_DONE, c); }
  bool out_landed(int) { return true; }
  void drain() { log.push_back({DRAIN, 0}); }
};

// ---- a call ------------------------------------------------------------------------------------------------------------------
static constexpr size_t kUnit = 21;  // bytes of a frame of the contiguous-range job

struct Call {
  bool range = false;  // frames of kUnit bytes through submit_range, else M rows of floats through submit
  int M = 1, N = 1;    // input rows (a range job: the bytes of a frame it reads), output rows
  int distinct = 0;    // the M row pointers go round this many rows of samples (0: a row each)
  HostChunkPlan plan;
  bool nt = true, staged_in = true, staged_out = true;
  bool hold_last = false;  // the output transfer of the chunk before the failing one ends only after the failing step has failed
  Inject inj;
  size_t n() const { return plan.cstart[plan.nch]; }
};

static HostChunkPlan plan_of(int nch, size_t len, size_t last) {
  HostChunkPlan p;
  p.short_call = false;
  p.nch = nch;
  p.cb = 0;
  for (int c = 0; c < nch; c++) p.cstart[c] = (size_t)c * len;
  p.cstart[nch] = (size_t)(nch - 1) * len + last;
  return p;
}
// the plans of the sweep: 1, 2 and 11 chunks with a ragged last one, and as many as a plan holds
static HostChunkPlan sweep_plan(int nch) {
  return nch == 1 ? plan_of(1, 1201, 1201) : nch == 2 ? plan_of(2, 640, 333) : nch == 11 ? plan_of(11, 112, 37) : plan_of(nch, 2700 / nch + 1, 5);
}

// y[i] = state = state / 2 + a[i] + b[i] / 4: the one function the chunks and the expected result both run
template <typename T>
static void recur(float *state, const T *a, const T *b, size_t stride, float *y, size_t len) {
  float s = *state;
  for (size_t i = 0; i < len; i++) y[i] = s = 0.5f * s + (float)a[i * stride] + 0.25f * (float)b[i * stride];
  *state = s;
}

struct Input {
  std::vector<std::vector<float>> rows;
  std::vector<const float *> ptrs;
  std::vector<unsigned char> bytes;
  Input(const Call &k, unsigned seed) {
    uint32_t lcg = seed * 2654435761u + 1u;
    const auto next = [&lcg] { return (lcg = lcg * 1664525u + 1013904223u) >> 8; };
    if (k.range) {
      bytes.resize(k.n() * kUnit);
      for (auto &v : bytes) v = (unsigned char)next();
    } else {
      rows.assign(k.distinct ? k.distinct : k.M, std::vector<float>(k.n()));
      for (auto &r : rows)
        for (auto &v : r) v = (float)((int)(next() & 0xffff) - 32768) * (1.0f / 32768.0f);
      for (int m = 0; m < k.M; m++) ptrs.push_back(rows[m % rows.size()].data());
    }
  }
  // output row j over the whole call, in one piece
  std::vector<float> expected(const Call &k, int j) const {
    std::vector<float> y(k.n());
    float state = 0.0f;
    const int a = j % k.M, b = (j + 1) % k.M;
    if (k.range) recur(&state, bytes.data() + a % kUnit, bytes.data() + b % kUnit, kUnit, y.data(), k.n());
    else recur(&state, ptrs[a], ptrs[b], 1, y.data(), k.n());
    return y;
  }
};

static const float kSentinel = -77777.0f;
static bool same_bits(const float *a, const float *b, size_t n) { return std::memcmp(a, b, n * sizeof(float)) == 0; }

// One pool, one set of lanes and their buffers, kept from call to call as a renderer keeps them.
struct Pipeline {
  std::unique_ptr<GatherPool> pool;
  ThreadLanes lanes;
  std::vector<float> p_in, d_in, d_out, p_out, state;
  std::vector<unsigned char> p_bytes, d_bytes;
  int chunks_run = -1;
  explicit Pipeline(int nthreads) : pool(new GatherPool) { pool->start(nthreads); }

  // the call through the real loop, into out[N] rows of n samples; throws what the loop throws
  void run(const Call &k, const Input &x, float *const *out) {
    const size_t n = k.n();
    const int M = k.M, N = k.N;
    const HostChunkPlan &plan = k.plan;
    // (every call has inputs of its own, so what an earlier call left in the input buffers would show)
    if (p_in.size() < n * M) p_in.resize(n * M), d_in.resize(n * M);
    if (p_bytes.size() < n * kUnit) p_bytes.resize(n * kUnit), d_bytes.resize(n * kUnit);
    d_out.assign(n * N, kSentinel), p_out.assign(n * N, kSentinel);
    state.assign(N, 0.0f);
    lanes.log.clear();
    lanes.inj = k.inj;
    lanes.set_gate(!k.hold_last);
    chunks_run = -1;
    const auto chunk = [&plan](size_t at) {
      int c = 0;
      while (plan.cstart[c] != at) c++;
      return c;
    };
    GatherPool *gp = nullptr;
    if (k.staged_in) {
      gp = pool.get();
      if (k.range) gp->submit_range(x.bytes.data(), p_bytes.data(), kUnit, plan.cstart, plan.nch, false, k.nt);
      else gp->submit(x.ptrs.data(), p_in.data(), n, plan.cstart, plan.nch, M, false, k.nt);
    }
    run_host_chunks(
        lanes, gp, plan, k.staged_out, &chunks_run,
        [&](size_t at, size_t len) {
          const Status s = lanes.step(H2D, chunk(at));
          if (!(s == Status())) return s;
          if (k.range) {
            const unsigned char *src = k.staged_in ? p_bytes.data() : x.bytes.data();
            lanes.in.push([=] { std::memcpy(d_bytes.data() + at * kUnit, src + at * kUnit, len * kUnit); });
          } else if (k.staged_in) {
            lanes.in.push([=] { std::memcpy(d_in.data() + M * at, p_in.data() + M * at, sizeof(float) * M * len); });
          } else {  // (rows the device reaches: a strided transfer straight from them)
            lanes.in.push([=, &x] {
              for (int m = 0; m < M; m++) std::memcpy(d_in.data() + M * at + m * len, x.ptrs[m] + at, sizeof(float) * len);
            });
          }
          return s;
        },
        [&](size_t at, size_t len) {
          const int c = chunk(at);
          lanes.log.push_back({KERNELS, c});
          if (k.inj.at(KERNELS, c)) {
            lanes.set_gate(true);
            if (k.inj.std_exception) throw std::runtime_error("the kernels threw at chunk " + std::to_string(c));
            throw Error{EARHIP_DEVICE_ERROR, "the kernels failed at chunk " + std::to_string(c)};
          }
          lanes.compute.push([=] {
            for (int j = 0; j < N; j++) {
              const int a = j % M, b = (j + 1) % M;
              float *y = d_out.data() + N * at + j * len;
              if (k.range) recur(&state[j], d_bytes.data() + at * kUnit + a % kUnit, d_bytes.data() + at * kUnit + b % kUnit, kUnit, y, len);
              else recur(&state[j], d_in.data() + M * at + a * len, d_in.data() + M * at + b * len, 1, y, len);
            }
          });
        },
        [&](size_t at, size_t len) {
          const int c = chunk(at);
          const Status s = lanes.step(D2H, c);
          if (!(s == Status())) return s;
          if (k.hold_last && c == k.inj.chunk - 1) lanes.out.push([this] { lanes.wait_at_gate(); });
          if (k.staged_out) {
            lanes.out.push([=] { std::memcpy(p_out.data() + N * at, d_out.data() + N * at, sizeof(float) * N * len); });
          } else {
            lanes.out.push([=] {
              for (int j = 0; j < N; j++) std::memcpy(out[j] + at, d_out.data() + N * at + j * len, sizeof(float) * len);
            });
          }
          return s;
        },
        [&](size_t at, size_t len) {
          lanes.log.push_back({SCATTER, chunk(at)});
          for (int j = 0; j < N; j++) std::memcpy(out[j] + at, p_out.data() + N * at + j * len, sizeof(float) * len);
        },
        [] { return 0.0; });
  }
  bool pool_finished() {
    std::lock_guard<std::mutex> lk(pool->mu);
    return pool->generation == 0 || pool->finished == pool->nthreads();  // (no job yet, or all threads through it)
  }
};

// the order in which a call of n chunks asks for its stages: all of them for every chunk in turn, up to and with the one that
// fails, then one drain
static std::vector<Ev> expected_order(int n, const Inject &inj) {
  std::vector<Ev> want;
  for (int c = 0; c < n; c++)
    for (Op op : {H2D, IN_DONE, KERNELS, KERNELS_DONE, D2H, OUT_DONE}) {
      want.push_back({op, c});
      if (inj.at(op, c)) goto drain;
    }
drain:
  want.push_back({DRAIN, 0});
  return want;
}

static std::string describe(const Call &k, int threads) {
  char s[200];
  snprintf(s, sizeof s, "%s M %d N %d threads %d chunks %d n %zu nt %d staged in %d out %d inject %s at %d%s", k.range ? "range" : "rows", k.M, k.N,
           threads, k.plan.nch, k.n(), (int)k.nt, (int)k.staged_in, (int)k.staged_out, kOpName[k.inj.op], k.inj.chunk, k.hold_last ? " (out lane held)" : "");
  return s;
}

// One call, all of it checked: a call that should succeed gives the expected rows bit for bit; one made to fail stops where it
// should, leaves the pool and the lanes idle, hands back nothing it should not, and reports what was injected.  The output rows
// are made for the call and freed right after it.  Returns the scatters made while the loop waited for the gather.
static int run_and_check(Pipeline &p, const Call &k, unsigned seed) {
  const std::string what = describe(k, p.pool->nthreads());
  const Input x(k, seed);
  const int nch = k.plan.nch;
  std::vector<std::unique_ptr<float[]>> rows;
  std::vector<float *> out;
  for (int j = 0; j < k.N; j++) {
    rows.emplace_back(new float[k.n()]);
    std::fill(rows.back().get(), rows.back().get() + k.n(), kSentinel);
    out.push_back(rows.back().get());
  }
  g_last_error.clear();
  const int rc = guarded([&] { p.run(k, x, out.data()); });
  // whatever happened: nothing of the call is left behind
  CHECK(p.pool_finished(), "%s: the pool has not finished its job", what.c_str());
  CHECK(p.lanes.idle(), "%s: a lane is not idle", what.c_str());
  std::vector<Ev> order, scatters;
  size_t last_stage = 0, last_scatter = 0;
  for (size_t i = 0; i < p.lanes.log.size(); i++) {
    const Ev &e = p.lanes.log[i];
    (e.op == SCATTER ? scatters : order).push_back(e);
    if (e.op == SCATTER) last_scatter = i;
    else if (e.op != DRAIN) last_stage = i;
  }
  CHECK(order == expected_order(nch, k.inj), "%s: %zu stages asked for, in another order than expected", what.c_str(), order.size());
  const bool fails = k.inj.op != NONE;
  const int done = !k.staged_out ? 0 : fails ? k.inj.chunk : nch;  // chunks that may come back through scatter
  for (size_t i = 0; i < scatters.size(); i++)
    CHECK(scatters[i].c == (int)i && (int)i < done, "%s: scatter %zu is of chunk %d", what.c_str(), i, scatters[i].c);
  int in_loop = 0;
  for (size_t i = 0; i < p.lanes.log.size(); i++)
    if (p.lanes.log[i].op == SCATTER && i < last_stage) in_loop++;
  if (!fails) {
    CHECK(rc == EARHIP_OK, "%s: status %d '%s'", what.c_str(), rc, g_last_error.c_str());
    CHECK(p.chunks_run == nch, "%s: chunks_run %d", what.c_str(), p.chunks_run);
    CHECK((int)scatters.size() == done, "%s: %zu scatters", what.c_str(), scatters.size());
    for (int j = 0; j < k.N; j++)
      CHECK(same_bits(out[j], x.expected(k, j).data(), k.n()), "%s: row %d differs", what.c_str(), j);
  } else {
    const std::string at = std::to_string(k.inj.chunk);
    const bool threw = k.inj.op == KERNELS;
    const std::string text = !threw ? kInjectedText : k.inj.std_exception ? "the kernels threw at chunk " + at : "the kernels failed at chunk " + at;
    CHECK(rc == (threw ? EARHIP_INTERNAL_ERROR : EARHIP_DEVICE_ERROR) && g_last_error == text, "%s: status %d '%s'", what.c_str(), rc,
          g_last_error.c_str());
    CHECK(p.chunks_run == -1, "%s: chunks_run %d", what.c_str(), p.chunks_run);
    CHECK(scatters.empty() || last_scatter < last_stage, "%s: a scatter after the failing step", what.c_str());
    // rows: what was handed back is right, everything else untouched
    for (int j = 0; j < k.N; j++) {
      const std::vector<float> want = x.expected(k, j);
      const size_t cut = k.plan.cstart[scatters.size()];
      CHECK(same_bits(out[j], want.data(), cut), "%s: row %d differs in the chunks handed back", what.c_str(), j);
      for (size_t i = cut; i < k.n(); i++)
        if (!same_bits(&out[j][i], &kSentinel, 1)) {
          CHECK(false, "%s: row %d sample %zu written though its chunk was not handed back", what.c_str(), j, i);
          break;
        }
    }
  }
  g_cases++;
  return in_loop;
}

// ---- the cases ---------------------------------------------------------------------------------------------------------------
static void sweep() {
  unsigned seed = 1;
  for (int threads : {1, 3, 8}) {
    Pipeline p(threads);
    for (int range = 0; range < 2; range++)
      for (int M : {1, 2, 5, 17, 37})
        for (int nch : {1, 2, 11, (int)HostChunkPlan::kMaxChunks})
          for (int nt = 0; nt < 2; nt++)
            for (int io = 0; io < 4; io++) {
              if (!(io & 1) && (threads != 1 || nt != 1)) continue;  // (without a gather its threads and stores make no other case)
              Call k;
              k.range = range != 0, k.M = k.N = M, k.plan = sweep_plan(nch), k.nt = nt != 0;
              k.staged_in = (io & 1) != 0, k.staged_out = (io & 2) != 0;  // (io 0: no gather and no scatter)
              run_and_check(p, k, seed++);
            }
  }
}

static void back_to_back(Pipeline &p, unsigned seed, int calls) {
  for (int i = 0; i < calls; i++) {
    static const int kChunks[] = {1, 7, 64, 3, 2, 33, 11, 1, 64, 5};
    Call k;
    k.range = i % 3 == 2, k.M = 1 + (i * 7) % 11, k.N = 1 + (i * 5) % 7, k.nt = i % 2 == 0;
    k.plan = plan_of(kChunks[i % 10], 37 + (size_t)(i % 4) * 16, 1 + (size_t)i % 29);
    run_and_check(p, k, seed + (unsigned)i);
  }
}

static void two_at_once() {
  std::thread other([] {
    Pipeline p(3);
    back_to_back(p, 5000, 20);
  });
  Pipeline p(2);
  back_to_back(p, 6000, 20);
  other.join();
}

static void pool_lifetime() {
  for (int threads : {1, 3, 8}) {
    {
      GatherPool pool;
      pool.start(threads);
    }
    g_cases++;
    for (int waits = 0; waits < 2; waits++) {  // (destroyed behind a finished job, and behind one it has only just been given)
      const HostChunkPlan plan = plan_of(5, 100, 41);
      std::vector<float> row(plan.cstart[5], 0.25f), staged(3 * plan.cstart[5], kSentinel);
      const float *in[3] = {row.data(), row.data(), row.data()};
      {
        GatherPool pool;
        pool.start(threads);
        pool.submit(in, staged.data(), plan.cstart[5], plan.cstart, 5, 3, false, true);
        if (waits) pool.wait_all();
      }
      bool whole = true;
      for (float v : staged) whole = whole && v == 0.25f;
      CHECK(!waits || whole, "pool of %d threads: the job it was destroyed behind is incomplete", threads);
      g_cases++;
    }
  }
}

// Each failing call stands between a good call of 8 chunks (every mark reached: stale) and another that must be right bit for
// bit.  The gather is made slow and the device quick: one staging thread copies 4096 short row pieces a chunk (the pointers go
// round five rows) for two rows of kernel work, so the loop is still waiting for the gather, polling, when a chunk's outputs land
// and after a stage has failed.
static void injected_failures() {
  Pipeline p(1);
  unsigned seed = 9000;
  int in_loop = 0, failing = 0;
  Call good;
  good.M = 4096, good.distinct = 5, good.N = 2, good.plan = plan_of(8, 64, 40);
  for (int chunk : {0, 2, 7})
    for (int kind = 0; kind < 7; kind++) {
      static const Op kOps[] = {H2D, IN_DONE, KERNELS_DONE, OUT_DONE, KERNELS, KERNELS, D2H};
      run_and_check(p, good, seed++);
      Call bad = good;
      bad.inj.op = kOps[kind], bad.inj.chunk = chunk, bad.inj.std_exception = kind == 5;
      in_loop += run_and_check(p, bad, seed++);
      failing++;
      // the same with a slow out lane: the chunk before the failing one lands only once the step has failed, while the loop still
      // polls for the gather of the chunks behind it: it must not come back
      if (chunk == 2) {
        run_and_check(p, good, seed++);
        bad.hold_last = true;
        in_loop += run_and_check(p, bad, seed++);
        failing++;
      }
    }
  run_and_check(p, good, seed++);
  printf("%d failing calls, %d chunks handed back while they waited for the gather\n", failing, in_loop);
  CHECK(in_loop > 0, "no failing call handed a chunk back while it waited for the gather: the stale marks were never asked about");
}

static void call_order() {
  for (int n : {1, 2, 11, (int)HostChunkPlan::kMaxChunks}) {
    RecordingLanes lanes;
    const HostChunkPlan plan = sweep_plan(n);
    const auto chunk = [&plan](size_t at) {
      int c = 0;
      while (plan.cstart[c] != at) c++;
      return c;
    };
    int chunks_run = -1;
    run_host_chunks(
        lanes, nullptr, plan, false, &chunks_run, [&](size_t at, size_t) { return lanes.step(H2D, chunk(at)); },
        [&](size_t at, size_t) { lanes.log.push_back({KERNELS, chunk(at)}); }, [&](size_t at, size_t) { return lanes.step(D2H, chunk(at)); },
        [&](size_t at, size_t) { lanes.log.push_back({SCATTER, chunk(at)}); }, [] { return 0.0; });
    CHECK(lanes.log == expected_order(n, Inject()) && chunks_run == n, "call order of %d chunks (%zu entries)", n, lanes.log.size());
    g_cases++;
  }
}

int main() {
  call_order();
  pool_lifetime();
  sweep();
  {
    Pipeline p(3);
    back_to_back(p, 4000, 50);
  }
  two_at_once();
  injected_failures();
  printf("%d cases, %d failed\n", g_cases.load(), g_failed.load());
  return g_failed.load() ? 1 : 0;
}
