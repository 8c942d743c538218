// How deep the compute waves' register ring really is, from the static schedules alone (plain C++, compiled with g++ by
// tests/test_step_ring_depth.py; tests/test_step_ring_isa.py holds the built kernels' s_waitcnt against these figures).
// For every register-fed slot of a block, in processing order: the number of LATER tile requests of the same wave that the schedule has
// raised by the time the slot is contracted.  A request is the 2 NCH loads of a tile's two weight rows, issued whether the workgroup has the
// tile or not (zn_step_kernel.h, load_into), so a wave that contracts such a slot may wait with vmcnt(2 NCH x that number) and leave the
// later tiles in flight.
//   * whole-step kernels: StepSched (zn_step_sched.h) with the shipped ZN_SK_NBUF = 3, ZN_SK_PARK = 2, ZN_SK_HELP = 0, ZN_CH_DEFER_MASK = 0xF,
//     ZN_SK_EARLY = 1 of six compute waves; step_r1_kernel runs the same three schedules.  Parked tiles (LDS) are not register-fed.
//     The same three schedules are first replayed for hazards by tests/step_schedule_check.cpp's replay().
//   * chain_kernel: its schedule is written out in the kernel (zn_chain_kernel.h: INIT requests at the start, the rest of the first
//     ZN_CH_NBUF behind op 0's publish, request l + NB raised by the last use of request l's buffer, held back behind the publish when it
//     is for another op) and repeated here; op 1 re-reads op 0's register buffers, so its slots count too.
// One line per instantiation: "<kernel template arguments>: op:d op:d ..." (the slot's op 0 .. 4 and its figure).  Exit status 0 unless a schedule is inconsistent.
#define main zn_shipped_schedules_main
#include "step_schedule_check.cpp"
#undef main

template <int T_OUT, int T_FC1, int T_FC2, int T_IN, int NB, int P, int NH, int MASK, int EARLY>
static void step_depths(const char* name) {
  using SC = StepSched<T_OUT, T_FC1, T_FC2, T_IN, NB, P, NH, MASK, EARLY>;
  std::vector<int> at(SC::NL, -1);             // position of each load's request in the wave's request order
  int n = 0;
  auto request = [&](int l) { if (l < 0 || l >= SC::NL || at[l] >= 0) { ++fails; std::printf("FAIL %s: request of load %d\n", name, l); return; } at[l] = n++; };
  auto item = [&](int i) { if (i < P) request(i); else if (i - P < SC::NREG) request(SC::nth_reg(i - P)); };      // [transit 0 .. P-1, REG 0 ..]
  for (int i = 0; i < NB; ++i) item(i);
  for (int l = 0; l < P; ++l) item(l + NB);     // behind each park store, the next item into the buffer just drained
  std::printf("%s:", name);
  for (int s = 0; s < SC::NS; ++s) {
    const int op = SC::op_of(s);
    if (s == SC::first_of(op) && op > 0)
      for (int q = SC::first_of(op - 1); q < SC::first_of(op); ++q)
        if (SC::raise_late(q)) request(SC::nth_reg(SC::raised_by(q)));
    const int l = SC::load_of_slot(s);
    if (SC::src_of(l) == 0) {
      if (at[l] < 0) { ++fails; std::printf(" FAIL(slot %d contracts a tile never requested)", s); }
      std::printf(" %d:%d", op, n - at[l] - 1);
      if (SC::raise_now(s)) request(SC::nth_reg(SC::raised_by(s)));
    }
  }
  std::printf("\n");
}

template <int T_OUT, int T_FC1, int T_FC2, int T_IN, int NB, int MASK>
static void chain_depths(const char* name) {
  constexpr int S1 = T_OUT, S2 = 2 * T_OUT, S3 = S2 + T_FC1, S4 = S3 + T_FC2, NS = S4 + T_IN;
  constexpr int NL = NS - T_OUT, INIT = T_OUT + 1 < NB ? T_OUT + 1 : NB;
  auto op_of = [](int s) { return s < S1 ? 0 : s < S2 ? 1 : s < S3 ? 2 : s < S4 ? 3 : 4; };
  auto first_of = [](int op) { return op == 0 ? 0 : op == 1 ? S1 : op == 2 ? S2 : op == 3 ? S3 : S4; };
  auto slot_of_load = [](int l) { return l < S1 ? l : l + T_OUT; };
  auto raised_by = [&](int s) { if (op_of(s) == 0) return -1; const int l = (s - T_OUT) + NB; return l < NL ? l : -1; };
  std::vector<int> at(NL, -1);
  int n = 0;
  auto request = [&](int l) { if (l < 0 || l >= NL || at[l] >= 0) { ++fails; std::printf("FAIL %s: request of load %d\n", name, l); return; } at[l] = n++; };
  for (int l = 0; l < INIT; ++l) request(l);
  std::printf("%s:", name);
  for (int s = 0; s < NS; ++s) {
    const int op = op_of(s);
    if (s == first_of(op) && op > 0) {
      if (op == 1) for (int l = INIT; l < (NL < NB ? NL : NB); ++l) request(l);
      if ((MASK >> (op - 1)) & 1)
        for (int q = first_of(op - 1); q < first_of(op); ++q) { const int l = raised_by(q); if (l >= 0 && op_of(slot_of_load(l)) != op - 1) request(l); }
    }
    const int here = op == 0 ? s : s - T_OUT;
    if (at[here] < 0) { ++fails; std::printf(" FAIL(slot %d contracts a tile never requested)", s); }
    std::printf(" %d:%d", op, n - at[here] - 1);
    const int l = raised_by(s);
    if (l >= 0 && ((((MASK >> op) & 1) == 0) || op_of(slot_of_load(l)) == op)) request(l);
  }
  for (int l = 0; l < NL; ++l) if (at[l] < 0) { ++fails; std::printf(" FAIL(load %d never requested)", l); }
  std::printf("\n");
}

int main() {
  replay<1, 7, 4, 4, 3, 2, 0, 0xF, 1>("replay step_kernel<4,1,7,4,4,6>");
  replay<1, 8, 4, 5, 3, 2, 0, 0xF, 1>("replay step_kernel<4,1,8,4,5,8>");
  replay<2, 9, 5, 5, 3, 2, 0, 0xF, 1>("replay step_kernel<4,2,9,5,5,12>");
  step_depths<1, 7, 4, 4, 3, 2, 0, 0xF, 1>("step<4,1,7,4,4,6>");
  step_depths<1, 8, 4, 5, 3, 2, 0, 0xF, 1>("step<4,1,8,4,5,8>");
  step_depths<2, 9, 5, 5, 3, 2, 0, 0xF, 1>("step<4,2,9,5,5,12>");
  chain_depths<1, 8, 4, 5, 3, 0xF>("chain<4,1,8,4,5>");
  chain_depths<1, 8, 4, 0, 3, 0xF>("chain<4,1,8,4,0>");
  chain_depths<1, 8, 4, 2, 3, 0xF>("chain<4,1,8,4,2>");
  chain_depths<1, 2, 1, 5, 3, 0xF>("chain<1,1,2,1,5>");
  chain_depths<1, 2, 1, 0, 3, 0xF>("chain<1,1,2,1,0>");
  chain_depths<1, 2, 1, 1, 3, 0xF>("chain<1,1,2,1,1>");
  return fails ? 1 : 0;
}
