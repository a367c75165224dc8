// firmix.h — the plan of the FIR filter matrix (include/earhip.h, group M) as plain C++ that the device kernels
// (firmix_kernels.h), the C ABI (api_firmix.hip) and a plain C++ program on the CPU (tests/cpp/firmix_host.cpp) all compile:
// the argument checks, the partition count, the lists of non-zero pairs, the ring of input spectra and the state sizes.
// No HIP header is needed to include it.
//
//   - uniformly partitioned convolution at the block size B: P = ceil(n_taps / B) partitions, the last one zero-padded;
//   - overlap-save: the transform of input block t is that of the 2B window [x_{t-1} | x_t], so the only state beside the
//     spectra is ONE block of input per channel (double-buffered: the workgroup of a call's last block rewrites it);
//   - the spectra of the windows live in a ring of R = max_blocks + P - 1 slots per channel: a call of n <= max_blocks blocks
//     writes n slots and reads back P - 1 slots behind its first, which are never the slots it writes;
//   - a pair (k, c) whose taps are all zero has no spectra and is in no list; an input channel without a pair has no ring
//     row and is never read; two outputs share one workgroup and one inverse transform (output 2g in the real part, 2g + 1
//     in the imaginary part), so the lists are kept per GROUP of two outputs: one entry per input channel that either needs.
#pragma once
#include <cmath>
#include <cstddef>
#include <vector>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define EARHIP_FIRMIX_HD __host__ __device__
#else
#define EARHIP_FIRMIX_HD
#endif

namespace earhip {

constexpr int kFirmixMaxIn = 64, kFirmixMaxOut = 64;
constexpr int kFirmixMinBlock = 64, kFirmixMaxBlock = 4096;
constexpr int kFirmixMaxParts = 64;

// nullptr when the configuration is one the matrix takes, else what is wrong with it (EARHIP_INVALID_ARGUMENT at create)
inline const char *firmix_check_config(int n_in, int n_out, int block, int n_taps, int max_blocks) {
  if (n_in < 1 || n_in > kFirmixMaxIn) return "n_in must be in [1, 64]";
  if (n_out < 1 || n_out > kFirmixMaxOut) return "n_out must be in [1, 64]";
  if (block < kFirmixMinBlock || block > kFirmixMaxBlock || (block & (block - 1)) != 0)
    return "block_size must be a power of two in [64, 4096]";
  if (n_taps < 1 || (long long)n_taps > (long long)kFirmixMaxParts * block) return "n_taps must be in [1, 64 * block_size]";
  if (max_blocks < 1) return "max_blocks must be >= 1";
  return nullptr;
}

inline bool firmix_taps_finite(const float *taps, size_t n) {
  for (size_t i = 0; i < n; i++)
    if (!std::isfinite(taps[i])) return false;
  return true;
}

EARHIP_FIRMIX_HD inline int firmix_partitions(int n_taps, int block) { return (n_taps + block - 1) / block; }
EARHIP_FIRMIX_HD inline int firmix_ring_slots(int partitions, int max_blocks) { return max_blocks + partitions - 1; }

// Ring slot of the window of block i - p, i the block's index in a call whose first block went to slot0.  i in
// [0, max_blocks), p in [0, P): slot0 + i - p lies in (-R, 2R).
EARHIP_FIRMIX_HD inline int firmix_ring_slot(int slot0, int i, int p, int R) {
  int s = slot0 + i - p;
  if (s < 0) s += R;
  if (s >= R) s -= R;
  return s;
}
// Partitions of block i of a call that reach a block fed since create / reset: p <= i + history, history = blocks fed
// before the call (what is older is zero and skipped, so the ring is never cleared)
EARHIP_FIRMIX_HD inline int firmix_live_partitions(int P, int i, unsigned long long blocks_before) {
  const unsigned long long have = (unsigned long long)i + blocks_before + 1ull;
  return have < (unsigned long long)P ? (int)have : P;
}

// one input channel of a group of two outputs: its ring row and the spectra of its two pairs (-1: that pair is all zero)
struct FirmixEntry {
  int row, h0, h1;
};

struct FirmixPlan {
  int n_in = 0, n_out = 0, block = 0, n_taps = 0, partitions = 0, ring = 0;
  int n_pairs = 0;                      // non-zero pairs = blocks of spectra [P][B]
  std::vector<int> used;                // input channels with a non-zero pair, ascending: ring row r holds channel used[r]
  std::vector<int> row_of;              // [n_in]: ring row of a channel, -1: never read
  std::vector<std::vector<int>> pairs;  // per output: its input channels, ascending (the summation order)
  std::vector<int> pair_index;          // [n_out][n_in]: which block of spectra, -1: none; numbered by output, then channel
  std::vector<int> group_start;         // [ceil(n_out / 2) + 1] into entries
  std::vector<FirmixEntry> entries;     // per group, ascending channel

  int groups() const { return (n_out + 1) / 2; }
  size_t spectra_elems() const { return (size_t)n_pairs * (size_t)partitions * (size_t)block; }  // complex numbers
  size_t ring_elems() const { return used.size() * (size_t)ring * (size_t)block; }               // complex numbers
  size_t state_elems() const { return 2 * used.size() * (size_t)block; }                         // floats, both halves
};

// taps [n_out][n_in][n_taps]; the configuration has passed firmix_check_config
inline FirmixPlan firmix_make_plan(int n_in, int n_out, int block, int n_taps, int max_blocks, const float *taps) {
  FirmixPlan p;
  p.n_in = n_in, p.n_out = n_out, p.block = block, p.n_taps = n_taps;
  p.partitions = firmix_partitions(n_taps, block);
  p.ring = firmix_ring_slots(p.partitions, max_blocks);
  p.row_of.assign((size_t)n_in, -1);
  p.pair_index.assign((size_t)n_out * (size_t)n_in, -1);
  p.pairs.resize((size_t)n_out);
  std::vector<char> needed((size_t)n_in, 0);
  for (int k = 0; k < n_out; k++)
    for (int c = 0; c < n_in; c++) {
      const float *h = taps + ((size_t)k * (size_t)n_in + (size_t)c) * (size_t)n_taps;
      bool any = false;
      for (int j = 0; j < n_taps && !any; j++) any = h[j] != 0.0f;  // (-0.0 is zero)
      if (!any) continue;
      p.pair_index[(size_t)k * (size_t)n_in + (size_t)c] = p.n_pairs++;
      p.pairs[(size_t)k].push_back(c);
      needed[(size_t)c] = 1;
    }
  for (int c = 0; c < n_in; c++)
    if (needed[(size_t)c]) {
      p.row_of[(size_t)c] = (int)p.used.size();
      p.used.push_back(c);
    }
  for (int g = 0; g < p.groups(); g++) {
    p.group_start.push_back((int)p.entries.size());
    const int k0 = 2 * g, k1 = 2 * g + 1;
    for (int c = 0; c < n_in; c++) {
      FirmixEntry e;
      e.row = p.row_of[(size_t)c];
      e.h0 = p.pair_index[(size_t)k0 * (size_t)n_in + (size_t)c];
      e.h1 = k1 < n_out ? p.pair_index[(size_t)k1 * (size_t)n_in + (size_t)c] : -1;
      if (e.h0 >= 0 || e.h1 >= 0) p.entries.push_back(e);
    }
  }
  p.group_start.push_back((int)p.entries.size());
  return p;
}

// ---- filter sets (earhip_firmix_create_sets) ------------------------------------------------------------------------------
// A matrix with room for n_sets filter sets of one shape.  Which set comes next is not known at create, so every input channel
// has a ring row (row = channel) and every set has spectra at full width: pair (k, c) of a set is block k n_in + c of the
// set's slice [n_out n_in][P][B], whether it is in the set's lists or not.  The lists are per set, with room for a dense set.
constexpr int kFirmixMaxSets = 4096, kFirmixMaxFade = 64;

struct FirmixSetLists {
  int n_pairs = 0;
  std::vector<int> group_start;      // [groups + 1] into entries
  std::vector<FirmixEntry> entries;  // per group, ascending channel; row = channel, h = k n_in + c
};
inline size_t firmix_set_entries_room(int n_in, int n_out) { return (size_t)((n_out + 1) / 2) * (size_t)n_in; }

// taps [n_out][n_in][n_taps]: all-zero pairs are dropped as in firmix_make_plan; taps == nullptr (the taps are in device
// memory, the host never sees them): no pair is dropped
inline FirmixSetLists firmix_make_set_lists(int n_in, int n_out, int n_taps, const float *taps) {
  FirmixSetLists s;
  const int groups = (n_out + 1) / 2;
  auto nonzero = [&](int k, int c) {
    if (k >= n_out) return false;
    if (!taps) return true;
    const float *h = taps + ((size_t)k * (size_t)n_in + (size_t)c) * (size_t)n_taps;
    for (int j = 0; j < n_taps; j++)
      if (h[j] != 0.0f) return true;
    return false;
  };
  for (int g = 0; g < groups; g++) {
    s.group_start.push_back((int)s.entries.size());
    for (int c = 0; c < n_in; c++) {
      const bool z0 = nonzero(2 * g, c), z1 = nonzero(2 * g + 1, c);
      FirmixEntry e;
      e.row = c;
      e.h0 = z0 ? (2 * g) * n_in + c : -1;
      e.h1 = z1 ? (2 * g + 1) * n_in + c : -1;
      s.n_pairs += (z0 ? 1 : 0) + (z1 ? 1 : 0);
      if (z0 || z1) s.entries.push_back(e);
    }
  }
  s.group_start.push_back((int)s.entries.size());
  return s;
}

// One step of the walk over the merged ascending channel lists of two sets (the fade kernel reads each X[c] once for both):
// the next channel that either list has, with the spectra of its up to four pairs (-1: none), and both cursors moved on.
struct FirmixMerged {
  int row, a0, a1, b0, b1;
};
EARHIP_FIRMIX_HD inline FirmixMerged firmix_merge_step(const FirmixEntry *ea, int &ia, int ea_end, const FirmixEntry *eb, int &ib,
                                                       int eb_end) {
  const int ra = ia < ea_end ? ea[ia].row : 0x7fffffff, rb = ib < eb_end ? eb[ib].row : 0x7fffffff;
  FirmixMerged m;
  m.row = ra < rb ? ra : rb;
  m.a0 = m.a1 = m.b0 = m.b1 = -1;
  if (ra == m.row) m.a0 = ea[ia].h0, m.a1 = ea[ia].h1, ia++;
  if (rb == m.row) m.b0 = eb[ib].h0, m.b1 = eb[ib].h1, ib++;
  return m;
}

// The fade schedule: host integers, advanced by every feed (a process call, a chunk of a pipelined render call, a span).
//   select(set, F): from the next block fed, `total` = F blocks go from the set that was current to `set`; afterwards `set`
//   alone.  While a fade is pending or running `current` is its target and `from` the set it leaves.
struct FirmixFade {
  int current = 0, from = -1, done = 0, total = 0;
};
// nullptr when select(set, F) is accepted, else why not (EARHIP_INVALID_ARGUMENT, nothing changed); loaded: [n_sets]
inline const char *firmix_select_check(const FirmixFade &f, int n_sets, const char *loaded, int set, int F) {
  if (set < 0 || set >= n_sets) return "set index out of range";
  if (F < 0 || F > kFirmixMaxFade) return "fade_blocks must be in [0, 64]";
  if (!loaded[set]) return "the set is not loaded";
  if (f.from >= 0 && f.done > 0) return "a fade has started and not finished";
  return nullptr;
}
// an accepted select.  A select before any block of the previous one was fed replaces it: `from` stays.
inline void firmix_select_apply(FirmixFade &f, int set, int F) {
  const int from = f.from >= 0 ? f.from : f.current;
  f.current = set;
  f.done = 0;
  if (F == 0 || set == from) f.from = -1, f.total = 0;  // a hard switch at the block boundary / nothing to fade between
  else f.from = from, f.total = F;
}
// how many of the next n blocks are fade blocks: always the first ones of a feed
EARHIP_FIRMIX_HD inline int firmix_fade_blocks(int from, int done, int total, int n) {
  if (from < 0) return 0;
  return n < total - done ? n : total - done;
}
inline void firmix_fade_advance(FirmixFade &f, int nfade) {
  f.done += nfade;
  if (f.from >= 0 && f.done >= f.total) f.from = -1, f.done = 0, f.total = 0;
}
inline void firmix_fade_end(FirmixFade &f) { f.from = -1, f.done = 0, f.total = 0; }  // reset: the target is current
// a set that may not be loaded now: the current one (a fade's target included) and the one being faded from
inline bool firmix_set_in_use(const FirmixFade &f, int set) { return set == f.current || set == f.from; }
// the weight of the target at sample n of fade block q of F blocks of B: starts at 0, never reaches 1 (q B + n < 2^24: exact)
EARHIP_FIRMIX_HD inline float firmix_fade_gain(int q, int n, int F, int B) { return (float)(q * B + n) / (float)(F * B); }

}  // namespace earhip
