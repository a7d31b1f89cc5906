// Driver of tests/test_pool_mirror_cpu.py: xivo_amd/csrc/pool_mirror.h alone, compiled with g++ -std=c++17 (no HIP). Each scenario
// prints "step key=value ..." lines that the test reads. Shapes: 2 filters, pool_max 3, anchor_max 2, group slots 0..2; every
// scenario works on filter 1 and prints both filters, so an index that drops its filter term shows.
#include <cstdio>
#include <cstring>

#include "pool_mirror.h"

using xivo_hip::capi::PoolMirror;

static const int NB = 2, PM = 3, AM = 2;

// every cell: e<b><i> the anchor of entry i of filter b, a<b><k> the link of its anchor k
static void cells(const char* step, const PoolMirror& m) {
  printf("%s", step);
  for (int b = 0; b < NB; ++b) for (int i = 0; i < PM; ++i) printf(" e%d%d=%d", b, i, m.entry_anchor(b, i));
  for (int b = 0; b < NB; ++b) for (int k = 0; k < AM; ++k) printf(" a%d%d=%d", b, k, m.anchor_link(b, k));
  printf("\n");
}

static int life() {
  PoolMirror m;
  printf("unconfigured empty=%d pm=%d am=%d exists=%d free=%d\n", (int)m.empty(), m.pool_max(), m.anchor_max(), (int)m.anchor_exists(0, 0), m.entry_anchor(0, 0));
  m.configure(NB, PM, AM);
  cells("fresh", m);
  printf("fresh_q empty=%d pm=%d am=%d\n", (int)m.empty(), m.pool_max(), m.anchor_max());
  // xivo_hip_pool_add's rule: the anchor exists (never created: refused; created and unlinked: fine)
  printf("add_rule never=%d", (int)m.anchor_exists(1, 1));
  m.anchor_created(1, 1);
  printf(" unlinked=%d other_filter=%d other_anchor=%d empty=%d\n", (int)m.anchor_exists(1, 1), (int)m.anchor_exists(0, 1), (int)m.anchor_exists(1, 0), (int)m.empty());
  m.configure(NB, PM, AM);
  m.entry_added(1, 2, 1);
  printf("entry_only empty=%d anchor=%d other_filter=%d\n", (int)m.empty(), m.entry_anchor(1, 2), m.entry_anchor(0, 2));
  // out of range: free / never created, whatever the index
  printf("range e_hi=%d e_lo=%d b_hi=%d a_hi=%d a_lo=%d linked=%d slot=%d\n", m.entry_anchor(1, PM), m.entry_anchor(1, -1), m.entry_anchor(NB, 0),
         m.anchor_link(1, AM), m.anchor_link(1, -1), (int)m.anchor_linked(NB, 0), (int)m.slot_linked(NB, 0));
  m.configure(0, 0, 0);
  printf("released empty=%d pm=%d am=%d\n", (int)m.empty(), m.pool_max(), m.anchor_max());
  return 0;
}

// the pool of the edit scenarios: filter 1 has anchors 0 and 1 created, entry 0 on anchor 0, entry 1 on anchor 1; filter 0 has
// anchor 0 created and linked to slot 1 (the same slot the scenarios use in filter 1)
static void prepared(PoolMirror& m) {
  m.configure(NB, PM, AM);
  m.anchor_created(1, 0); m.anchor_created(1, 1);
  m.entry_added(1, 0, 0); m.entry_added(1, 1, 1);
  m.anchor_created(0, 0);
  PoolMirror::Edit e(m);
  e.group_anchored(0, 1, 0);
  e.commit();
}

static int edits() {
  PoolMirror m;
  prepared(m);
  cells("prepared", m);
  // xivo_hip_pool_anchor's refusal: a linked anchor cannot be created again (an unlinked one can)
  printf("recreate linked=%d unlinked=%d\n", (int)m.anchor_linked(0, 0), (int)m.anchor_linked(1, 0));
  // group anchored: the same slot in the other filter does not interfere; refused on an anchor that is not unlinked (never
  // created: a fresh pool's; linked: after the edit) and on a slot another anchor of the filter holds
  PoolMirror fresh;
  fresh.configure(NB, PM, AM);
  printf("anchor_rule ok=%d never=%d", (int)m.can_anchor_group(1, 1, 0), (int)fresh.can_anchor_group(1, 1, 0));
  printf(" admit_free=%d admit_unlinked=%d", (int)m.can_admit(1, 2), (int)m.can_admit(1, 0));
  {
    PoolMirror::Edit e(m);
    e.group_anchored(1, 1, 0);
    printf(" again=%d slot_taken=%d other_slot=%d admit_linked=%d admit_other=%d", (int)m.can_anchor_group(1, 2, 0), (int)m.can_anchor_group(1, 1, 1),
           (int)m.can_anchor_group(1, 2, 1), (int)m.can_admit(1, 0), (int)m.can_admit(1, 1));
    e.commit();
  }
  printf("\n");
  cells("anchored", m);
  // group removed: every anchor that links the slot, and no other (filter 0 links the same slot)
  {
    PoolMirror::Edit e(m);
    e.group_anchored(1, 2, 1);
    e.group_removed(1, 1);
    e.commit();
  }
  cells("removed", m);
  return 0;
}

// [anchor a0 -> slot 1, admit entry 0, remove group 1, bad op]: the Edit is left without commit; the same list without the bad op
// commits
static int transaction() {
  PoolMirror m;
  prepared(m);
  cells("before", m);
  int ok[3] = {0, 0, 0};
  for (int pass = 0; pass < 2; ++pass) {
    {
      PoolMirror::Edit e(m);
      ok[0] = m.can_anchor_group(1, 1, 0);
      e.group_anchored(1, 1, 0);
      ok[1] = m.can_admit(1, 0);       // relies on the link the op before made
      e.entry_admitted(1, 0);
      if (pass == 0) cells("linked_admitted", m);
      e.group_removed(1, 1);
      if (pass == 0) cells("removed", m);
      ok[2] = m.can_admit(1, 0);       // the bad op: the entry is free now
      if (pass == 1) e.commit();       // (pass 0 is the refused call: the destructor puts the mirrors back)
    }
    cells(pass == 0 ? "rolled_back" : "committed", m);
  }
  printf("ops anchor=%d admit=%d bad=%d\n", ok[0], ok[1], ok[2]);
  m.entry_added(1, 2, 1);            // outside an Edit nothing is journalled: a later refused Edit undoes only its own ops
  {
    PoolMirror::Edit e(m);
    e.group_anchored(1, 2, 1);
    e.entry_admitted(1, 2);
    cells("second_inside", m);
  }
  cells("second_rolled_back", m);
  return 0;
}

static int dead() {
  PoolMirror m;
  m.configure(NB, PM, AM);
  m.anchor_created(0, 0); m.anchor_created(1, 0);
  for (int b = 0; b < NB; ++b) for (int i = 0; i < PM; ++i) m.entry_added(b, i, 0);
  const unsigned char live1[PM] = {1, 0, 1};                 // B = 1: filter 1 is not part of the step
  m.entries_dead(live1, 1);
  cells("one_filter", m);
  const unsigned char live2[NB * PM] = {1, 1, 1, 0, 1, 0};
  m.entries_dead(live2, 2);
  cells("both", m);
  return 0;
}

struct Ent { int ref_sind; };
struct Anc { int slot; };

static int reread() {
  PoolMirror m;
  m.configure(NB, PM, AM);
  m.anchor_created(0, 1); m.entry_added(0, 0, 1);            // stale: the device says otherwise
  const Ent ent[NB * PM] = {{-1}, {-1}, {-1}, {1}, {AM}, {-7}};          // filter 1: anchor 1, past the last anchor, negative
  const Anc anc[NB * AM] = {{-1}, {-1}, {-1}, {2}};
  const int used[NB * AM] = {0, 0, 1, 1};                    // filter 0: a slot of an unused anchor is not read
  m.reread(ent, anc, used);
  cells("reread", m);
  const Anc anc2[NB * AM] = {{2}, {-1}, {-1}, {2}};
  const int used2[NB * AM] = {0, 1, 0, 1};
  m.reread(ent, anc2, used2);
  cells("unused_with_slot", m);
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  if (!strcmp(argv[1], "life")) return life();
  if (!strcmp(argv[1], "edits")) return edits();
  if (!strcmp(argv[1], "transaction")) return transaction();
  if (!strcmp(argv[1], "dead")) return dead();
  if (!strcmp(argv[1], "reread")) return reread();
  return 2;
}
