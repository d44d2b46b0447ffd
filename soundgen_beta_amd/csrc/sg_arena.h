// sg_arena.h — the sections of a plan's HBM arena, declared once. Every device
// array of a synthesis plan is one row of SG_ARENA; the arena pointers
// (ArenaPtrs, the base of DevicePlan), the per-section element counts
// (ArenaCounts), the offsets and the total (arena_each) are generated from it.
// Host code without the HIP runtime.
#pragma once
#include <algorithm>
#include <string>

#include "sg_dev.h"
#include "sg_plan.h"

namespace sg {

inline int64_t arena_tasks(const Batch& B) { return bulk_size(B.tasks_x, B.tasks); }
// fl: the uploaded floats, then the device-computed envelopes from fe_base on, then the
// noise uniforms expanded at upload from fu_base on
inline int64_t arena_fl(const Batch& B) {
  return std::max<int64_t>(std::max<int64_t>(bulk_size(B.fl_x, B.fl), B.fe_base + B.fe_total), B.fu_base + B.fu_total);
}

// X(name, element type, element count of the Batch B, extra bytes), in arena order
#define SG_ARENA(X)                                                                                    \
  X(segs, SgSeg, bulk_size(B.segs_x, B.segs), 0)                                                       \
  X(epochs, SgEpoch, B.epochs.size(), 0)                                                               \
  X(knots, double, B.knots.size(), 0)                                                                  \
  X(amps, float, B.amp_total, 64 * sizeof(float)) /* built on the device (sg_amp_build) */             \
  X(ampcols, const SgAmpCol, B.ampcols.size(), 0) /* sg_amp_build inputs (read at upload) */           \
  X(ampjobs, const SgAmpJob, B.ampjobs.size(), 0)                                                      \
  X(ampsrc, const float, B.ampsrc.size(), 0)                                                           \
  X(tasks, SgWTask, arena_tasks(B), 0)                                                                 \
  X(tall, int32_t, arena_tasks(B), 0)   /* indices of tasks with R > SG_ROWS_F32 (sg_sine_bank_tall) */ \
  X(tlong, int32_t, arena_tasks(B), 0)  /* fp32 tasks run one per wave (sg_sine_bank) */               \
  X(tshort, int32_t, arena_tasks(B), 0) /* fp32 tasks of <= 64 samples, two per wave (sg_sine_bank_pairs) */ \
  X(tallp, int32_t, arena_tasks(B), 0)  /* tall tasks of <= 64 samples (sg_sine_bank_tall_pairs) */    \
  /* runs of the two short lists: consecutive entries of one syllable, <= SG_RUN_TASKS each, one */    \
  /* wave per run (positions in tshort / tallp where each run starts, then the list size) */           \
  X(srun, int32_t, arena_tasks(B) + 1, 0)                                                              \
  X(trun, int32_t, arena_tasks(B) + 1, 0)                                                              \
  X(thp, int32_t, arena_tasks(B), 0)                      /* SG_TASK_HP tasks (sg_sine_bank_hp) */     \
  X(fin_tiles_hp, SgSylTile, B.fin_tiles_hp.size(), 0)    /* finalize tiles of fp64 syllables */       \
  X(W64, double, B.w64_total, 0)                          /* fp64 epoch waveforms of SG_TASK_HP tasks */ \
  X(fh, double, B.fh_total, 0)                            /* fp64 sounds of fp64 bouts */              \
  X(frames64, SgFrame64, B.frames64.size(), 0)            /* their filter frames (sg_fft_frames64) */  \
  X(frames64_tab, int64_t, B.frames64_tab.size(), 0)      /* per frame: offset of its root table */    \
  X(roots64, double, 2 * B.roots64_total, 0)              /* W_N^t tables (double2), one per window length */ \
  X(roots64_wl, int32_t, B.roots64_wl.size(), 0)                                                       \
  X(roots64_off, int64_t, B.roots64_off.size(), 0)                                                     \
  X(pieces, SgPiece, B.pieces.size(), 0)                                                               \
  X(syls, SgSyllable, B.syls.size(), 0)                                                                \
  X(syl_tiles, SgSylTile, B.fin_tiles.size(), 0)          /* general-path finalize tiles (Batch::fin_tiles) */ \
  X(copy_tiles, SgCopyTile, B.copy_tiles.size(), 0)                                                    \
  X(ptiles, SgSylTile, B.ptiles.size(), 0)                                                             \
  X(cknots, double, B.cknots.size(), 0)                                                                \
  X(W, float, B.w_total, 0)                                                                            \
  X(taskmax, float, arena_tasks(B), 0)                                                                 \
  X(ptilemax, float, B.ptiles.size(), 0)                                                               \
  X(maxes, float, B.syls.size(), 0)                                                                    \
  X(geoms, SgFftGeom, B.geoms.size(), 0)                                                               \
  X(frames, SgFrame, B.frames[0].size() + B.frames[1].size(), 0) /* noise frames, then filter frames */ \
  X(fgroups, SgFrameGroup, B.fgroups.size(), 0)                                                        \
  X(olas, SgOla, B.olas_dev.size(), 0)                                                                 \
  X(olatiles, SgOlaTile, B.olatiles.size(), 0)                                                         \
  X(olasegs, SgSegment, B.olasegs.size(), 0)                                                           \
  X(olatilemax, float, B.olatiles.size() + (size_t)B.n_segslots, 0) /* tile slots, then segment slots */ \
  X(olamax, float, B.olas_dev.size(), 0)                                                               \
  X(items, SgNoiseItem, B.items.size(), 0)                                                             \
  X(mixes, SgMix, B.mixes_dev.size(), 0)                                                               \
  X(mixtiles, SgMixTile, B.mixtiles.size(), 0)                                                         \
  X(eterms, SgEnvTerm, bulk_size(B.eterms_x, B.eterms), 0)                                             \
  X(ecols, SgEnvCol, B.ecols.size(), 0)                                                                \
  X(envjobs, SgEnvJob, B.envjobs.size(), 0)                                                            \
  X(envtasks, SgEnvTask, B.envtasks.size(), 0)                                                         \
  X(elog2, double, B.elog2.size(), 0)                                                                  \
  X(fl, float, arena_fl(B), 0)                                                                         \
  X(fs, float, B.fs_total, 256)

// the arena pointers, one per section
struct ArenaPtrs {
#define X(name, T, count, extra) T* name = nullptr;
  SG_ARENA(X)
#undef X
};

// the elements each section was sized for
struct ArenaCounts {
#define X(name, T, count, extra) int64_t name = 0;
  SG_ARENA(X)
#undef X
};
inline ArenaCounts arena_counts(const Batch& B) {
  ArenaCounts n;
#define X(name, T, count, extra) n.name = (int64_t)(count);
  SG_ARENA(X)
#undef X
  return n;
}

// Every section starts on a multiple of 256 B; an empty one still takes 256 B
constexpr size_t SG_ARENA_ALIGN = 256;
inline size_t arena_up(size_t x) { return (x + SG_ARENA_ALIGN - 1) / SG_ARENA_ALIGN * SG_ARENA_ALIGN; }

// f(name, the section's pointer in P, element count, offset, bytes taken) for every
// section in arena order; returns the arena's size
template <class F>
size_t arena_each(const ArenaCounts& n, ArenaPtrs& P, F&& f) {
  size_t o = 0;
#define X(name, T, count, extra)                                                 \
  {                                                                              \
    const size_t bytes = (size_t)n.name * sizeof(T) + (extra);                   \
    const size_t take = arena_up(bytes > 0 ? bytes : 1);                         \
    f(#name, P.name, n.name, o, take);                                           \
    o += take;                                                                   \
  }
  SG_ARENA(X)
#undef X
  return o;
}
inline size_t arena_bytes(const ArenaCounts& n) {
  ArenaPtrs none;
  return arena_each(n, none, [](const char*, auto*&, int64_t, size_t, size_t) {});
}
// P's pointers into the arena at base
inline void arena_point(const ArenaCounts& n, char* base, ArenaPtrs& P) {
  arena_each(n, P, [&](const char*, auto*& p, int64_t, size_t off, size_t) {
    p = reinterpret_cast<std::remove_reference_t<decltype(p)>>(base + off);
  });
}

// The bytes of a copy of n elements to element `at` of a section that holds `count`
// elements of `elem` bytes. A copy that does not fit throws and names the section.
inline size_t arena_copy_bytes(const char* name, size_t elem, int64_t count, int64_t at, int64_t n) {
  if (at < 0 || n < 0 || at > count || n > count - at)
    throw SgError(SG_E_DEVICE, std::string("arena section ") + name + ": " + std::to_string(n) + " elements at " +
                                   std::to_string(at) + " do not fit its " + std::to_string(count));
  return (size_t)n * elem;
}

}  // namespace sg
