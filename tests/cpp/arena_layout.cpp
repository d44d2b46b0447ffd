// arena_layout — the sections of a plan's HBM arena (sg_arena.h) for hand-filled
// batches, as the host compiler builds them without the HIP runtime.
// tests/test_planner.py builds this with g++ and recomputes every offset from the
// printed counts with its own table of element sizes.
//
// Prints, for each of three batches (each of the three terms of fl's size the
// largest in one of them): "run K", "NAME OFFSET BYTES COUNT" per section in arena
// order, "total N"; then the copy check's lines: "copy NAME fits BYTES" or
// "copy NAME refused CODE MESSAGE".
#include <cstdio>
#include <cstring>

#include "sg_arena.h"

using namespace sg;

// every array a different small size; several empty
static Batch make_batch(int run) {
  Batch B;
  B.segs_x.blocks.resize(2);  // two blocks and a tail
  B.segs_x.blocks[0].resize(5);
  B.segs_x.blocks[1].resize(9);
  B.segs_x.base = {0, 5};
  B.segs_x.n = 14;
  B.segs.resize(3);
  B.epochs.resize(7);
  B.knots.resize(33);
  B.amp_total = 1000;
  B.ampcols.resize(11);
  B.ampjobs.resize(6);
  // ampsrc empty
  B.tasks_x.blocks.resize(2);
  B.tasks_x.blocks[0].resize(4);
  B.tasks_x.blocks[1].resize(2);
  B.tasks_x.base = {0, 4};
  B.tasks_x.n = 6;
  B.tasks.resize(7);
  B.fin_tiles_hp.resize(2);
  B.w64_total = 515;
  B.fh_total = 0;  // empty
  B.frames64.resize(3);
  B.frames64_tab.resize(3);
  B.roots64_total = 70;
  B.roots64_wl.resize(2);
  B.roots64_off.resize(2);
  B.pieces.resize(19);
  B.syls.resize(5);
  B.fin_tiles.resize(8);
  // copy_tiles empty
  B.ptiles.resize(13);
  // cknots empty
  B.w_total = 4099;
  B.geoms.resize(2);
  B.frames[0].resize(10);
  B.frames[1].resize(21);
  B.fgroups.resize(4);
  B.olas_dev.resize(6);
  B.olatiles.resize(17);
  B.olasegs.resize(12);
  B.n_segslots = 9;
  B.items.resize(15);
  B.mixes_dev.resize(5);
  B.mixtiles.resize(23);
  B.eterms_x.blocks.resize(1);
  B.eterms_x.blocks[0].resize(30);
  B.eterms_x.base = {0};
  B.eterms_x.n = 30;
  B.eterms.resize(1);
  B.ecols.resize(14);
  // envjobs, envtasks empty
  B.elog2.resize(129);
  B.fl.resize(700);
  // run 0: the uploaded floats end last; 1: the envelope area; 2: the uniform area
  B.fe_base = run == 0 ? 600 : 700;
  B.fe_total = run == 1 ? 260 : 50;
  B.fu_base = run == 1 ? 0 : B.fe_base + B.fe_total;
  B.fu_total = run == 2 ? 345 : run == 1 ? 0 : 20;
  B.fs_total = 2001;
  return B;
}

static void copy_check(const char* name, size_t elem, int64_t count, int64_t at, int64_t n) {
  try {
    std::printf("copy %s fits %zu\n", name, arena_copy_bytes(name, elem, count, at, n));
  } catch (const SgError& e) {
    std::printf("copy %s refused %d %s\n", name, e.code, e.what());
  }
}

int main() {
  for (int run = 0; run < 3; ++run) {
    const Batch B = make_batch(run);
    const ArenaCounts n = arena_counts(B);
    ArenaPtrs P;
    std::printf("run %d\n", run);
    const size_t total = arena_each(n, P, [](const char* name, auto*&, int64_t count, size_t off, size_t bytes) {
      std::printf("%s %zu %zu %lld\n", name, off, bytes, (long long)count);
    });
    std::printf("total %zu\n", total);
    if (total != arena_bytes(n)) return 1;
    // the pointers land on the printed offsets
    char* base = reinterpret_cast<char*>(uintptr_t(1) << 20);
    arena_point(n, base, P);
    bool ok = true;
    arena_each(n, P, [&](const char*, auto*& p, int64_t, size_t off, size_t) {
      ok = ok && reinterpret_cast<const char*>(p) == base + off;
    });
    if (!ok) return 2;
  }
  const ArenaCounts n = arena_counts(make_batch(0));
  copy_check("ptiles", sizeof(SgSylTile), n.ptiles, 0, n.ptiles);          // as many as it holds
  copy_check("ptiles", sizeof(SgSylTile), n.ptiles, 0, n.ptiles + 1);      // one more
  copy_check("frames", sizeof(SgFrame), n.frames, 10, 21);                 // the second phase behind the first
  copy_check("frames", sizeof(SgFrame), n.frames, 11, 21);
  copy_check("cknots", sizeof(double), n.cknots, 0, 0);                    // an empty section takes an empty copy
  copy_check("cknots", sizeof(double), n.cknots, 0, 1);
  return 0;
}
