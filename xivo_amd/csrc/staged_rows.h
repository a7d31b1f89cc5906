// The measurement rows currently staged in a context, as ONE record: how many there are, in which representations they
// are valid right now, and what the producer that left them has to tell the consumers ("Staged rows"). Host-only,
// plain C++17, no HIP: tests/staged_rows_driver.cpp replays every producer of the C ABI against this file alone.
//
// Representations of the rows of a filter:
//   row-pair compressed (ell.h)   fits(b); nc(b) / pw(b) bound the slots in use
//   dense H                       dense_alive()                    (else ensure_dense materialises it)
//   dense H^T                     dense_alive() && ht_alive()      (else ensure_HT)
//   mixed                         mixed_row0() >= 0: rows [0, mixed_row0) compressed only, the OOS rows behind them dense only
//   lead                          has_lead(): the calibration columns of the compressed rows live in the leading dense block
//
// The fields change through the named transitions below and nowhere else - one per thing that happens to the rows.
// Invariants (tests/test_staged_rows_cpu.py asserts them after every step of every producer sequence):
//   rows_padded() == rows() rounded up to 16
//   every producer of NEW rows (handed_over, stacked) clears lead, mixed_row0 and oos_row0: oos_row0() >= 0 only between an
//     OOS append and the next producer of rows
//   mixed_row0() >= 0  =>  !dense_alive() at the time of the append (get_H or the dense pipeline may materialise it later),
//     !dense_from_compressed(), !has_lead() and oos_row0() == mixed_row0()
//   has_lead()  =>  !dense_alive() and every filter of the stacking fits
//   dense_clean()  =>  no row of the dense buffer was written except by the mixed append itself
//   ht_alive() never claims more than the launches wrote (it may claim less: a redundant transpose is harmless)
// The record speaks for the WHOLE context: a hand-over of a sub-range [b0, b0 + nb) sets the row count and the flags of every
// filter and only the fit of its own; callers that hand over in pieces pass the same M each time.
#pragma once
#include <algorithm>
#include <vector>

namespace xivo_hip::capi {

enum class Stacking { in_state_as_coded, full_rows };   // full_rows: the whole J() of a masked set - cannot be re-stacked from the gate's mask
enum class CalibCols { none, lead_block, in_rows };     // where the calibration columns of stacked rows went (in_rows: they do not fit)
enum class GateLayout { packed, strided };              // row stride of mask / dist: F (dense-row gate inside the update) or Fmax

class StagedRows {
 public:
  struct Slots { int nc, pw; };   struct Restack { int B; double R; };

  // common / private slots of the compressed form: what a filter that does not fit is charged with
  void sized(int Bmax, int common, int priv) { cw_ = common; pwmax_ = priv; over_.assign(Bmax, 1); nc_.assign(Bmax, common); pw_.assign(Bmax, priv); }

  int rows() const { return M_; }                int rows_padded() const { return Mp_; }
  bool dense_alive() const { return dense_; }    bool ht_alive() const { return ht_; }
  bool dense_from_compressed() const { return from_ell_; }   // ensure_dense expands the compressed rows (else: re-stacks)
  bool dense_clean() const { return clean_; }    // every row of the dense buffer the mixed mode has not written itself is zero
  int mixed_row0() const { return mixed_row0_; } bool has_lead() const { return lead_; }
  int oos_row0() const { return oos_row0_; }     int oos_max_rows() const { return oos_max_rows_; }     double oos_R() const { return oos_R_; }
  bool fits(int b) const { return over_[b] == 0; }  int nc(int b) const { return nc_[b]; }  int pw(int b) const { return pw_[b]; }
  bool any_over(int b0, int nb) const { return std::any_of(over_.begin() + b0, over_.begin() + b0 + nb, [](int o) { return o != 0; }); }
  Slots max_slots(int b0, int nb) const {   // (at least one private slot; one pass of plain maxima: called per update with the whole batch)
    Slots s{0, 1}; for (int b = b0; b < b0 + nb; ++b) { s.nc = std::max(s.nc, nc_[b]); s.pw = std::max(s.pw, pw_[b]); } return s;
  }
  Restack restack_args() const { return {stack_B_, stack_R_}; }
  GateLayout gate_layout() const { return gate_; }

  // M rows per filter handed over as a dense matrix (set_measurements*, close_loop_stack, the one-filter call): compressed,
  // the fit of filters [b0, b0 + nb) follows through fit_reported; or (!compressed) dense rows and H^T written for all of them
  void handed_over(int b0, int nb, int M, bool compressed) {
    new_rows(M); dense_ = !compressed; from_ell_ = true; ht_ = true;
    for (int b = b0; !compressed && b < b0 + nb; ++b) fit_reported(b, 1, cw_, pwmax_ + 1);
  }
  // what the compression reports for filter b; a filter that does not fit gets its dense rows written next to the compressed ones
  void fit_reported(int b, int over, int nc, int pw) { over_[b] = over; nc_[b] = nc; pw_[b] = pw; if (over) clean_ = false; }
  // the scene's F features stacked for filters [0, B) with noise R (xivo_hip_stack, the whole-row stackings of the calibration
  // gate and RANSAC); dense: H and H^T written too. Full rows that fit keep the compressed form as the source of a later dense copy.
  // pw: private slots a pair uses (6: group + feature block as coded, 9: with the group block fixed / whole rows)
  void stacked(int B, int F, double R, Stacking kind, int pw, bool dense, CalibCols cc) {
    new_rows(2 * F);
    for (int b = 0; b < B; ++b) { over_[b] = cc == CalibCols::in_rows; nc_[b] = 12; pw_[b] = pw; }   // (12 common slots: sensor pose + extrinsics)
    lead_ = cc == CalibCols::lead_block; dense_ = dense; from_ell_ = kind == Stacking::full_rows && cc != CalibCols::in_rows; stack_B_ = B; stack_R_ = R;
    if (dense) { ht_ = true; clean_ = false; }
  }
  // up to max_rows OOS rows per filter appended behind the staged ones for filters [b0, b0 + nb); mixed: into the dense buffer
  // only (no H^T), the in-state rows stay compressed; else every row of those filters is dense now
  void oos_appended(int max_rows, double R, bool mixed, int b0, int nb) {
    oos_row0_ = M_; oos_R_ = R; oos_max_rows_ = max_rows; mixed_row0_ = mixed ? M_ : -1;
    if (mixed) ht_ = false; else std::fill_n(over_.begin() + b0, nb, 1);
    M_ += max_rows; Mp_ = (M_ + 15) & ~15;
  }
  // the OOS block QR-compressed in place to at most max_rows rows per filter (H^T is not rewritten in the mixed mode)
  void oos_compressed(int max_rows) {
    M_ = oos_row0_ + max_rows; Mp_ = (M_ + 15) & ~15; oos_max_rows_ = max_rows;
    if (mixed_row0_ >= 0) ht_ = false;
  }
  // ensure_dense issued its launch: mixed - the in-state rows expanded next to the OOS rows, H only; from the compressed rows -
  // H and H^T (ht_alive is left as it was); re-stacked - H and H^T
  void dense_materialised() {
    if (mixed_row0_ >= 0) ht_ = false; else if (!from_ell_) ht_ = true;
    dense_ = true; clean_ = false;
  }
  // ... of a lead stacking: the re-stacked dense rows carry the calibration columns, the compressed ones no longer stand alone
  void lead_demoted() { lead_ = false; std::fill_n(over_.begin(), stack_B_, 1); }
  // xivo_hip_set_calib changed the calibration layout under the stacking
  void lead_dropped() { lead_ = false; }
  // ensure_HT issued its launch
  void ht_materialised() { ht_ = true; }
  // every row of the dense buffer cleared ahead of a mixed append
  void dense_zeroed() { clean_ = true; }
  // a gate wrote mask / dist with this row stride
  void gate_wrote(GateLayout g) { gate_ = g; }

 private:
  void new_rows(int M) { M_ = M; Mp_ = (M + 15) & ~15; lead_ = false; mixed_row0_ = -1; oos_row0_ = -1; }

  int M_ = 0, Mp_ = 0, cw_ = 0, pwmax_ = 0, mixed_row0_ = -1, oos_row0_ = -1, oos_max_rows_ = 0, stack_B_ = 0;
  std::vector<int> over_, nc_, pw_;
  bool dense_ = true, from_ell_ = false, ht_ = true, clean_ = true, lead_ = false;   GateLayout gate_ = GateLayout::packed;
  double stack_R_ = 0.0, oos_R_ = 0.0;
};

}  // namespace xivo_hip::capi
