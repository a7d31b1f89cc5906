// Replays the producers of the C ABI (capi_update.hip / capi_glevel.hip) as transitions of StagedRows and prints the whole
// record after every step: tests/test_staged_rows_cpu.py holds the expected table. Compiled with g++ -std=c++17 against
// xivo_amd/csrc/staged_rows.h alone - no HIP, no device.
#include <cstdio>
#include <cstring>
#include <initializer_list>

#include "staged_rows.h"

using namespace xivo_hip::capi;

namespace {

constexpr int kB = 3, kCommon = 16, kPrivate = 12;   // filters; ELL_CW, ELL_PW of ell.h
constexpr int kF = 20;                               // features of the scene: 40 stacked rows

struct Ctx {
  StagedRows r;
  bool calib_on = false, dense_h = false, fix_group_block = false;
  int Mpmax = 112;   // rows allocated per filter
  bool calib_sparse() const { return calib_on && !dense_h; }
  Ctx() { r.sized(kB, kCommon, kPrivate); }
};

void show(const char* seq, const char* step, const Ctx& c) {
  const StagedRows& r = c.r;
  const auto [sB, sR] = r.restack_args();
  printf("%s/%s: %d %d %d %d %d %d %d %d %d %d %g %d %g %c |", seq, step, r.rows(), r.rows_padded(), (int)r.dense_alive(),
         (int)r.dense_from_compressed(), (int)r.ht_alive(), (int)r.dense_clean(), r.mixed_row0(), (int)r.has_lead(), r.oos_row0(),
         r.oos_max_rows(), r.oos_R(), sB, sR, r.gate_layout() == GateLayout::strided ? 'S' : 'P');
  for (int b = 0; b < kB; ++b) printf(" %d", (int)!r.fits(b));
  printf(" |");
  for (int b = 0; b < kB; ++b) printf(" %d", r.nc(b));
  printf(" |");
  for (int b = 0; b < kB; ++b) printf(" %d", r.pw(b));
  const auto ms = r.max_slots(0, kB);
  printf(" | %d %d %d\n", ms.nc, ms.pw, (int)r.any_over(0, kB));
}

// ---- the producers and materialisers, as the host code calls the transitions
void ensure_HT(Ctx& c) { if (!c.r.ht_alive()) c.r.ht_materialised(); }

void ensure_dense(Ctx& c) {
  StagedRows& r = c.r;
  if (r.dense_alive()) return;
  if (r.mixed_row0() < 0 && !r.dense_from_compressed() && r.has_lead()) r.lead_demoted();
  r.dense_materialised();
}

// stage_measurements: `over` per filter as the compression kernel reports it (pw 13: one private slot too many)
void hand_over(Ctx& c, int b0, int nb, int M, bool compressed, std::initializer_list<int> over = {}) {
  c.r.handed_over(b0, nb, M, compressed);
  int b = b0;
  for (int o : over) { c.r.fit_reported(b, o, o ? kCommon : 12, o ? kPrivate + 1 : 6); ++b; }
}

void dropin(Ctx& c, int b, int M) { c.r.handed_over(b, 1, M, true); c.r.fit_reported(b, 0, 12, 6); }

void mh_gate(Ctx& c) {
  c.r.gate_wrote(GateLayout::strided);
  if (c.calib_on && !c.calib_sparse()) {   // calib_gate: every present feature stacked as its whole row, dense
    c.r.stacked(kB, kF, 1.0, Stacking::full_rows, 9, true, CalibCols::in_rows);
    c.r.gate_wrote(GateLayout::strided);
  }
}

void stack(Ctx& c) {
  const CalibCols cc = !c.calib_on ? CalibCols::none : c.calib_sparse() ? CalibCols::lead_block : CalibCols::in_rows;
  c.r.stacked(kB, kF, 1.0, Stacking::in_state_as_coded, c.fix_group_block ? 9 : 6, c.dense_h || cc == CalibCols::in_rows, cc);
}

void ransac(Ctx& c) {
  const CalibCols cc = c.calib_on ? CalibCols::in_rows : CalibCols::none;
  c.r.stacked(kB, kF, 1.0, Stacking::full_rows, 9, c.dense_h || c.calib_on, cc);
  if (c.calib_on) c.r.stacked(kB, kF, 1.0, Stacking::full_rows, 9, true, cc);
  c.r.gate_wrote(GateLayout::strided);
}

void oos_project(Ctx& c, int max_rows) {
  StagedRows& r = c.r;
  const int M = r.rows(), pad = (max_rows + 16 + 15) & ~15;
  const bool mixed = !c.calib_on && !r.dense_alive() && !r.dense_from_compressed() && r.oos_row0() < 0 && !c.dense_h && M % 2 == 0 &&
                     M + pad <= c.Mpmax;
  if (!mixed) ensure_dense(c);
  else if (!r.dense_clean()) r.dense_zeroed();
  r.oos_appended(max_rows, 12.25, mixed, 0, kB);
}

// the update's effect on the record: the dense routes materialise the dense rows (and, gated or as coded, H^T); a gate inside
// the update leaves mask / dist packed
void update(Ctx& c, bool dense_route, bool gate = false) {
  if (dense_route) { ensure_dense(c); ensure_HT(c); }
  if (gate) c.r.gate_wrote(GateLayout::packed);
}

#define STEP(name, call) do { call; show(seq, name, c); } while (0)

void run(const char* seq) {
  Ctx c;
  show(seq, "created", c);
  if (!strcmp(seq, "handover_fit")) {
    STEP("hand_over", hand_over(c, 0, kB, 40, true, {0, 0, 0}));
    STEP("update", update(c, false));
    STEP("get_H", ensure_dense(c));
    STEP("hand_over_again", hand_over(c, 0, kB, 40, true, {0, 0, 0}));
  } else if (!strcmp(seq, "handover_mixed_batch")) {
    STEP("hand_over", hand_over(c, 0, kB, 40, true, {0, 1, 0}));
    STEP("update_dense", update(c, true));
    STEP("hand_over_sub_range", hand_over(c, 1, 1, 40, true, {0}));
  } else if (!strcmp(seq, "handover_none_fit")) {
    STEP("hand_over", hand_over(c, 0, kB, 40, false));
    STEP("update_dense", update(c, true));
  } else if (!strcmp(seq, "stack_oos")) {
    STEP("mh_gate", mh_gate(c));
    STEP("stack", stack(c));
    STEP("oos_project", oos_project(c, 20));
    STEP("compress_oos", c.r.oos_compressed(9));
    STEP("get_H", ensure_dense(c));
    STEP("oos_project_2", oos_project(c, 10));
    STEP("update_dense", update(c, true));
    STEP("stack_next_frame", stack(c));
    STEP("oos_project_resident", oos_project(c, c.r.oos_max_rows()));
  } else if (!strcmp(seq, "oos_no_spare_rows")) {
    c.Mpmax = 64;
    STEP("stack", stack(c));
    STEP("oos_project", oos_project(c, 20));
  } else if (!strcmp(seq, "stack_dense_h")) {
    c.dense_h = true; c.fix_group_block = true;
    STEP("stack", stack(c));
    STEP("gated_update", update(c, true, true));
    STEP("oos_project", oos_project(c, 20));
  } else if (!strcmp(seq, "calib_lead")) {
    c.calib_on = true;
    STEP("mh_gate", mh_gate(c));
    STEP("stack", stack(c));
    STEP("update", update(c, false));
    STEP("get_H", ensure_dense(c));
    STEP("stack_again", stack(c));
    STEP("update_dense_gated", update(c, true, true));
    STEP("set_calib", c.r.lead_dropped());
  } else if (!strcmp(seq, "calib_dense")) {
    c.calib_on = true; c.dense_h = true;
    STEP("mh_gate", mh_gate(c));
    STEP("stack", stack(c));
    STEP("ransac", ransac(c));
  } else if (!strcmp(seq, "ransac")) {
    STEP("hand_over", hand_over(c, 0, kB, 40, true, {0, 0, 0}));
    STEP("ransac", ransac(c));
    STEP("stack", stack(c));
    STEP("ransac_again", ransac(c));
    STEP("get_H", ensure_dense(c));
  } else if (!strcmp(seq, "close_loop")) {
    STEP("stack", stack(c));
    STEP("oos_project", oos_project(c, 20));
    STEP("close_loop_stack", hand_over(c, 0, kB, 8, true, {0, 0, 0}));
  } else if (!strcmp(seq, "handover_after_oos")) {
    STEP("stack", stack(c));
    STEP("oos_project", oos_project(c, 20));
    STEP("hand_over", hand_over(c, 0, kB, 40, true, {0, 0, 0}));
  } else if (!strcmp(seq, "dropin_after_lead")) {
    c.calib_on = true;
    STEP("stack", stack(c));
    STEP("dropin", dropin(c, 0, 30));
    STEP("stack_again", stack(c));
  } else if (!strcmp(seq, "dropin_and_batch")) {
    STEP("dropin", dropin(c, 1, 30));
    STEP("stack", stack(c));
    STEP("dropin_again", dropin(c, 1, 30));
  }
}

}  // namespace

int main(int argc, char** argv) {
  for (int i = 1; i < argc; ++i) run(argv[i]);
  return 0;
}
