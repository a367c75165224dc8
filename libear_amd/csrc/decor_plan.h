// decor_plan.h — the host-side decisions of the decorrelator stage (K2) of the renderer: how the FIRs are partitioned, which
// kernel runs them, how many blocks a run takes.  Plain C++ (no HIP): decor_stage.h acts on them, tests/cpp/test_decor_plan.cpp
// pins them against tests/golden/decor_plan.txt.
#pragma once

namespace earhip {

struct DecorPlan {
  // The decorrelators' own partition size Bk (and transform size Lk = 2 Bk).  A linear convolution does not
  // depend on how it is partitioned, so callers' blocks of 1024, 2048 ... samples run through 512-sample
  // partitions whenever the FIRs fit one of them: the wave kernel (k_decorrelate_wave) exists for that size
  // and is 2.5 times faster per sample than the workgroup kernel at 2048 points (BASELINE config 5: K2 0.125
  // -> 0.05 ms).  Otherwise Bk = B, libear's own partitioning (src/dsp/block_convolver_impl.cpp:16-41).
  int Bk = 0, Lk = 0;
  int NP = 1;                // partitions of the decorrelator FIRs (ceil(n_taps / Bk))
  int run_len = 11;          // blocks per decorrelator run of the workgroup kernel
  bool run_len_set = false;  // option RUN given: also fixes the run length of the wave kernel
};

// K buses, blocks of B samples, FIRs of n_taps; options K2_OWN_BLOCK and RUN (run_given: whether it is set at all)
inline DecorPlan decor_plan(int K, int B, int n_taps, bool own_block, bool run_given, int run) {
  DecorPlan p;
  p.Bk = B;
  if (K == 2 && B > 512 && B % 512 == 0 && n_taps <= 512 && !own_block) p.Bk = 512;
  p.Lk = 2 * p.Bk;
  p.NP = (n_taps + p.Bk - 1) / p.Bk;
  // workgroup decorrelator kernel: blocks per run.  Block 1024 (BASELINE config 5, 512 blocks x 24
  // loudspeakers): 7 -> K2 0.113 ms, 5 -> 0.117, 11 -> 0.128, 15 -> 0.140 (two rounds of workgroups that fill
  // the chip evenly beat one ragged round)
  if (p.Lk == 2048) p.run_len = 7;
  if (run_given && run >= 1 && run <= 255) p.run_len = run | 1, p.run_len_set = true;  // tuning knob: blocks per run (odd)
  return p;
}

// one wave per run (k_decorrelate_wave) or a workgroup per run (FIRs of several partitions, other sizes; option K2_WG)
inline bool decor_wave_kernel(const DecorPlan &p, bool k2_wg) { return p.Lk == 1024 && p.NP == 1 && !k2_wg; }

// Run length (odd, so that the warm-up block pairs with the first one) of k_decorrelate_wave for a
// call of T blocks on N loudspeakers, `waves` runs to a workgroup.  A run of R blocks costs (R+1)/2 pair transforms, each
// workgroup puts one wave on every SIMD, and a CU holds three workgroups (LDS): the cost of a
// round of k = 1..3 resident workgroups per CU is pairs x c[k] with the measured pair times
// c = 6.9, 9.3, 12.2 us (latency-bound at this occupancy).  NOTES.md (round 2, section 4, K2).
inline int wave_run_len(int T, int N, int num_cus, int waves) {
  const double c[4] = {0.0, 6.9, 9.3, 12.2};
  int best = 1;
  double best_cost = 1e30;
  for (int R = 1; R <= 31; R += 2) {
    const long runs = (T + R - 1) / R;
    const long wgs = (runs + waves - 1) / waves * N;
    const long full = wgs / (3L * num_cus), rem = wgs - full * 3L * num_cus;
    const double pairs = (R + 1) / 2;
    const double cost = pairs * (full * c[3] + c[(rem + num_cus - 1) / num_cus]);
    if (cost <= best_cost) best_cost = cost, best = R;  // (ties: the longer run does less warm-up work)
    if (runs == 1) break;
  }
  return best;
}

}  // namespace earhip
