// cc_solve_host.hpp -- the host side of driving an LM solve on the device, shared by the intrinsics and the rig handle
// (host code only; cc_intrinsics.hip and cc_rig.hip include it below their kernels). What differs between the solvers stays
// with them: what a round enqueues, how the pinned block is laid out, how the control block is read back, the persistent forms.
// The functions take a SolveHost*; the two that need the solver's device struct (h->d) are templates over the handle type.
#pragma once
#include <algorithm>
#include <chrono>
#include <cstring>
#include <string>
#include <vector>

#include "cc_common.hpp"
#include "cc_persist_publish.hpp"

namespace cc {

// RCCL, resolved lazily with dlopen so that single-GPU use never loads it (cc_comm.cpp)
struct Comm;
int comm_create(const uint8_t id[128], int rank, int nranks, Comm** out);
void comm_destroy(Comm* c);
int comm_allreduce_sum(Comm* c, double* buf, int n, hipStream_t stream);

struct SolveHost {   // base of cc_intrinsics and cc_rig
  int device = 0;
  hipStream_t stream = nullptr;
  void* pinned = nullptr;       // the pinned block host_pub and h_ctl live in (each solver lays it out: *_create_impl)
  volatile unsigned long long* host_pub = nullptr;   // [0] sequence word written by the device, [2..19] control block (rig: [20] failure word)
  unsigned long long pub_count = 0;                  // chunks published so far (what the sequence word will read next: + 1)
  LmCtl* h_ctl = nullptr;       // pinned
  LmOpts cached_opts{};         // what the device currently holds
  bool opts_valid = false;
  hipGraphExec_t graph[3] = {nullptr, nullptr, nullptr};   // captured chunks of check_interval = graph_iters (which is which: solve_launch, rig_launch)
  int graph_iters = 0;
  Comm* comm = nullptr;
  Mailbox mailbox;              // mailbox exchange (*_exchange_export / _attach): our mailbox and the peers' mappings
  bool exchange = false;
  std::vector<hipEvent_t> events;
  std::vector<int> event_kind;
  std::vector<int> event_round;   // round of the solve a probed launch belongs to (summarise_probes)
  int enq_round = 0;
  int ran_form = -1;            // the form the handle's LAST solve ran in to its end (-1: none yet, 0: one set of kernels per iteration, else what *_solver_form says)
  int form_reruns = 0;          // persistent solves that gave up and were run again in form 0 (*_solver_status)
  std::string form_note;        // why
};

// What every solve has, whichever solver runs it (SolveRun and RigRun add their own flags)
struct SolveRunBase {
  cc_options o;
  bool profile = false, use_graph = false;
  int launched = 0;
  LmCtl st{};
  std::chrono::steady_clock::time_point t0;
};

static void drop_graphs(SolveHost* h) {
  for (auto& g : h->graph)
    if (g) { hipGraphExecDestroy(g); g = nullptr; }
}

static void clear_probes(SolveHost* h) {
  for (auto e : h->events) hipEventDestroy(e);
  h->events.clear();
  h->event_kind.clear();
  h->event_round.clear();
  h->enq_round = 0;
}

struct Probe {  // optional hipEvent bracket around one launch
  SolveHost* h; int kind; bool on; int round_shift; hipEvent_t e0 = nullptr, e1 = nullptr;
  Probe(SolveHost* h_, int kind_, bool on_, int round_shift_ = 0) : h(h_), kind(kind_), on(on_), round_shift(round_shift_) {
    if (on) { hipEventCreate(&e0); hipEventCreate(&e1); hipEventRecord(e0, h->stream); }
  }
  ~Probe() {
    if (on) { hipEventRecord(e1, h->stream); h->events.push_back(e0); h->events.push_back(e1); h->event_kind.push_back(kind); h->event_round.push_back(h->enq_round + round_shift); }
  }
};

// One report to the device's back-off window (persist_device_try, cc_common.hpp) per probe it admitted: completed() and
// gave_up() act once, and a probe that is dropped without either -- an early return after it started -- has given up.
struct PersistProbe {
  int device, kind; bool open;
  PersistProbe(int device_, int kind_, bool admitted) : device(device_), kind(kind_), open(admitted) {}
  PersistProbe(const PersistProbe&) = delete;
  void completed() { if (open) persist_device_completed(device, kind); open = false; }
  void gave_up() { if (open) persist_device_gave_up(device, kind); open = false; }
  ~PersistProbe() { gave_up(); }
};

template <class H>
static int write_ctl(H* h, const LmCtl& c) {   // both copies of the control block
  CC_HIP(hipMemcpyAsync(h->d.ctl, &c, sizeof(c), hipMemcpyHostToDevice, h->stream));
  CC_HIP(hipMemcpyAsync(h->d.ctl_next, &c, sizeof(c), hipMemcpyHostToDevice, h->stream));
  return 0;
}

// Waits for the chunk just enqueued: spins on the sequence word its last kernel stores into pinned host memory (no copy
// engine, no stream synchronisation on the way), then takes the control block -- and, for a caller that passes `wait_failed`,
// the failure word of the in-kernel waits -- from next to it. A stream that has gone idle without the word showing up (a
// kernel fault, a stale counter) falls back to a copy: `read_ctl()`, the solver's own (it fills *c and *wait_failed).
// `stream2` (or NULL): the chunk is a lean persistent rig solve -- its ONLY publisher is the control workgroup on that second
// stream, and the workers on h->stream leave as soon as they have seen `done` in their boxes, a few microseconds BEFORE the
// control has written the control block and the sequence word. The fallback is therefore taken only when BOTH streams are
// idle (with h->stream alone the host could re-synchronise its count and read a half-written control block
// while the control workgroup was still publishing, and the late publication then satisfied the NEXT solve's wait at once).
// `who`: "the solver" / "the rig solver", for the message.
template <class ReadCtl>
static int wait_published(SolveHost* h, hipStream_t stream2, LmCtl* c, bool* wait_failed, const char* who, ReadCtl read_ctl) {
  const unsigned long long* word = const_cast<const unsigned long long*>(h->host_pub);
  const unsigned long long want = ++h->pub_count;
  for (unsigned spins = 0;; ++spins) {
    if (__atomic_load_n(word, __ATOMIC_ACQUIRE) == want) break;
    if ((spins & 0xfffu) == 0xfffu) {
      hipError_t q = hipStreamQuery(h->stream);
      if (q == hipSuccess && stream2) q = hipStreamQuery(stream2);
      if (q == hipSuccess) {
        if (__atomic_load_n(word, __ATOMIC_ACQUIRE) == want) break;
        h->pub_count = __atomic_load_n(word, __ATOMIC_ACQUIRE);
        return read_ctl();
      }
      if (q != hipErrorNotReady) return fail(CC_ERR_HIP, "stream failed while waiting for %s: %s", who, hipGetErrorString(q));
    }
  }
  std::memcpy(c, word + 2, sizeof(LmCtl));
  if (wait_failed) *wait_failed = h->host_pub[2 + sizeof(LmCtl) / 8] != 0ull;
  return 0;
}

// The same wait for a whole solve of the persistent intrinsics kernel, which publishes its control block as tagged words
// (cc_persist_publish.hpp) at host_pub + kPubTaggedAt: spins until a copy of the kPubWords words, taken word by word, carries the
// tag of the count this wait expects in every word, and reassembles the block from that copy. No word of the block is ordered
// against another, and none against the plain sequence word host_pub[0], which the kernel still stores: it is what the fallback
// -- the one of wait_published, unchanged -- resynchronises the count from once the stream has gone idle.
template <class ReadCtl>
static int wait_published_tagged(SolveHost* h, LmCtl* c, const char* who, ReadCtl read_ctl) {
  static_assert(sizeof(LmCtl) == kPubDoubles * 8, "the tagged publication carries the whole control block");
  const unsigned long long* word = const_cast<const unsigned long long*>(h->host_pub);
  const unsigned long long* tagged = word + kPubTaggedAt;
  const uint32_t want = publish_tag(++h->pub_count);
  unsigned long long copy[kPubWords];
  auto arrived = [&] {
    for (int i = kPubWords - 1; i >= 0; --i) {
      copy[i] = __atomic_load_n(tagged + i, __ATOMIC_RELAXED);
      if ((uint32_t)(copy[i] >> 32) != want) return false;
    }
    return publish_ready(copy, want);
  };
  for (unsigned spins = 0;; ++spins) {
    if (arrived()) break;
    if ((spins & 0xfffu) == 0xfffu) {
      const hipError_t q = hipStreamQuery(h->stream);
      if (q == hipSuccess) {
        if (arrived()) break;
        h->pub_count = __atomic_load_n(word, __ATOMIC_ACQUIRE);
        return read_ctl();
      }
      if (q != hipErrorNotReady) return fail(CC_ERR_HIP, "stream failed while waiting for %s: %s", who, hipGetErrorString(q));
    }
  }
  unsigned long long block[kPubDoubles];
  publish_unpack(copy, block);
  std::memcpy(c, block, sizeof(LmCtl));
  return 0;
}

// Captures what `enqueue()` puts on the handle's stream into an executable graph. On any failure the stream is taken out of
// capture mode again and nothing is kept (a stream left capturing would poison the process-wide stream cache it returns to).
template <class Enqueue>
static int capture_graph(SolveHost* h, hipGraphExec_t* out, Enqueue enqueue) {
  hipGraph_t g = nullptr;
  CC_HIP(hipStreamBeginCapture(h->stream, hipStreamCaptureModeThreadLocal));
  const int rc = enqueue();
  const hipError_t e_end = hipStreamEndCapture(h->stream, &g);
  if (rc || e_end != hipSuccess) {
    if (g) hipGraphDestroy(g);
    (void)hipGetLastError();
    return rc ? rc : fail(CC_ERR_HIP, "hipStreamEndCapture failed: %s", hipGetErrorString(e_end));
  }
  const hipError_t e_inst = hipGraphInstantiate(out, g, nullptr, nullptr, 0);
  hipGraphDestroy(g);
  if (e_inst != hipSuccess) { *out = nullptr; return fail(CC_ERR_HIP, "hipGraphInstantiate failed: %s", hipGetErrorString(e_inst)); }
  return 0;
}

// Head of a solve: the caller's options (or the defaults) clamped against the device log of `log_cap` records, probes of the
// last solve forgotten, graphs captured for another check_interval dropped. No stream work: that is the solver's own.
static int begin_common(SolveHost* h, const cc_options* opt, int log_cap, SolveRunBase* r) {
  r->t0 = std::chrono::steady_clock::now();
  if (opt) r->o = *opt; else cc_options_init(&r->o);
  cc_options& o = r->o;
  if (o.check_interval < 1) o.check_interval = 1;
  if (o.max_iterations > log_cap - 1) o.max_iterations = log_cap - 1;
  r->profile = o.profile_kernels != 0;
  r->use_graph = o.use_graph && !r->profile && !h->comm;
  r->launched = 0;
  CC_HIP(hipSetDevice(h->device));
  clear_probes(h);
  if (r->use_graph && h->graph_iters != o.check_interval) { drop_graphs(h); h->graph_iters = o.check_interval; }
  return 0;
}

// The options of a one-shot call (a handle made for ONE solve): the caller's, or the defaults -- the rig calls default to the
// reference's 1000 iterations (extrinsics_calibrator.cpp:211) -- and in either case no graph.
static cc_options one_shot_options(const cc_options* opt, int default_max_iterations = 0) {
  cc_options o;
  if (opt) o = *opt; else cc_options_init(&o);
  if (!opt && default_max_iterations) o.max_iterations = default_max_iterations;
  o.use_graph = 0;   // one solve per handle: capturing and instantiating a graph cannot pay off
  return o;
}

// The phases of a one-shot call for cc_last_call_timing (include/cc_solver.h: [0] handle + device arena, [1] upload, [2] the
// start, [3] solve, [4] read-back + teardown): every slot starts at 0 and mark(slot) adds the time since the last mark to it.
struct PhaseClock {
  double* tm = last_timing();
  std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
  PhaseClock() { for (int i = 0; i < 5; ++i) tm[i] = 0.0; }
  void mark(int slot) {
    const auto t1 = std::chrono::steady_clock::now();
    tm[slot] += std::chrono::duration<double, std::milli>(t1 - t0).count();
    t0 = t1;
  }
};

// The options are uploaded when they change, not per solve. true: the device must get `lo` (the caller stages the bytes its
// own way and sets opts_valid once they are on their way).
static bool opts_changed(SolveHost* h, const LmOpts& lo) {
  if (h->opts_valid && std::memcmp(&lo, &h->cached_opts, sizeof(lo)) == 0) return false;
  h->cached_opts = lo;
  h->opts_valid = false;
  return true;
}

template <class H>
static int finish_summary(H* h, const SolveRunBase* r, cc_summary* summary) {
  const LmCtl& st = r->st;
  CC_HIP(hipSetDevice(h->device));
  if (summary) {
    cc_iteration* user_log = summary->log;
    const int cap = summary->log_capacity;
    summary->iterations = st.iter;
    summary->successful_steps = st.n_success;
    summary->termination = st.term;
    summary->initial_cost = st.initial_cost;
    summary->final_cost = st.x_cost;
    summary->sweeps = st.sweeps;
    const int n = user_log ? std::min(std::min(st.log_len, cap), h->d.log_cap) : 0;
    summary->log_len = n;
    if (n > 0) CC_HIP(hipMemcpy(user_log, h->d.log, (size_t)n * sizeof(cc_iteration), hipMemcpyDeviceToHost));
    summarise_probes(h->events, r->profile ? h->event_kind : std::vector<int>(), h->event_round, st.iter, summary,
                     [](float* ms, hipEvent_t a, hipEvent_t b) { return hipEventElapsedTime(ms, a, b) == hipSuccess; });
    summary->seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - r->t0).count();
  }
  clear_probes(h);
  return CC_OK;
}

// *_solver_status behind its NULL check; form_now: what *_solver_form says
static int solver_status(const SolveHost* h, int form_now, int32_t* form, int32_t* reruns, char* note, int32_t note_capacity) {
  if (form) *form = form_now;
  if (reruns) *reruns = h->form_reruns;
  if (note && note_capacity > 0) std::snprintf(note, (size_t)note_capacity, "%s", h->form_note.c_str());
  return CC_OK;
}

// head of *_exchange_export (`who`: its name): nothing in flight, no graph, no mailbox, no exchange; the caller clears its d.x
static int exchange_export_begin(SolveHost* h, const void* handle, const char* who) {
  if (!h || !handle) return fail(CC_ERR_BAD_ARGUMENT, "%s: NULL argument", who);
  CC_HIP(hipSetDevice(h->device));
  CC_HIP(hipStreamSynchronize(h->stream));
  drop_graphs(h);
  mailbox_release(&h->mailbox);
  h->exchange = false;
  return 0;
}

}  // namespace cc
