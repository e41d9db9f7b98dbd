// kp_env.h — the KP_* environment variables of libkp.so and libkp_cpusim.so, and the two
// helpers every read of one goes through (tests/test_env_knobs.py holds the sources and
// this table to each other). Nothing is cached here: a variable is read where the table
// says, so the tests that flip one between two calls on the same engine see it take effect.
//
// Read:  process = once per process (a function-local static)
//        engine  = at kp_engine_create
//        batch   = at every kp_batch_create*
//        call    = at every schedule / explain call (or, for the CPU build, every launch)
// Use:   shipped = part of a measured configuration, test = a test's hook, tuning = for
//        measurement and diagnosis only
//
//   variable                 default   read     use      what it does
//   KP_STREAMS               3         engine   shipped  HIP streams per engine (1..3); batches in flight run with 1
//   KP_SYNC_BLOCK            0         process  shipped  1: host waits sleep in the driver instead of polling
//   KP_TOP                   1         engine   test     0: no k_select_top (the full-candidate kernels)
//   KP_TOP_CAP               832       engine   test     subset capacity of both k_select_top slices (64..1024)
//   KP_TOP_CAP_MID           0         engine   tuning   the large slice first at this capacity, its overflow at the full one
//   KP_TOP_SPLIT             1         engine   tuning   0: the two k_select_top slices on one stream
//   KP_TOP_SMALL_NEED        160       process  tuning   replicas + targets up to which a binding takes the small slice
//   KP_TOPK                  1         process  tuning   0: no histogram form of k_select_top (batches without class orders)
//   KP_SLOW_ORDER            1         engine   test     0: k_slow sorts its candidates instead of filtering the class order
//   KP_SLOW_GRID             (256)     batch    tuning   upper bound of k_slow's grid
//   KP_SLOW_LDS              1         batch    tuning   0: k_slow's sort keys and scale-down scratch stay in global memory
//   KP_WIDE_LDS              1         batch    test     0: k_region_wide's sort keys stay in global memory
//   KP_ORDER_AMORT           4         batch    test     bindings per estimator class below which a batch builds no class orders
//   KP_EST_SINGLE            1         process  tuning   0: singleton estimator classes keep whole rows
//   KP_SETS_RUNS_CAP         4096      batch    test     node runs per cluster of the component-set simulation (lowered only)
//   KP_ASSUME_RUNS_CAP       4096      call     test     node runs per cluster of kp_assumptions_create's deduction (lowered only)
//   KP_PACK_THREADS          (cpus)    batch    test     host threads that pack a batch
//   KP_PACK_TIMING           unset     batch    tuning   set: kp_batch_create prints its phase times to stderr
//   KP_PAIR_GENERIC          unset     call     test     set: the generic pair kernel whatever the snapshot allows
//   KP_PAIR_ROWS             unset     call     test     set: per-binding pair rows instead of k_filter + estimator classes
//   KP_REGION_HOST           unset     call     test     set: selectGroups on the host for every region binding
//   KP_REASONS_CHUNK         2^24      call     test     (binding, cluster) pairs per chunk of the reason rows
//   KP_DEBUG_SLOW            unset     call     tuning   set: the slow-path counters of every call on stderr
//   KP_SEL_THREADS           256       process  tuning   threads per workgroup of k_select_all (128, 256); set (seen per call): no wide instance
//   KP_CPUSIM_THREADS        1         call     test     CPU build: host threads that run a launch's workgroups
//   KP_CPUSIM_DEVICES        8         call     test     CPU build: emulated device count
//   KP_CPUSIM_POISON         1         process  test     CPU build: 0 leaves a workgroup's LDS unpoisoned
//   KP_CPUSIM_SLOW_SHUFFLE   unset     call     test     CPU build: seed that permutes k_slow's flagged list
//   KP_CPUSIM_SLOW_GRID      (grid)    call     test     CPU build: upper bound of k_slow's grid
//   KP_CPUSIM_LDS_SHRINK     0         call     test     CPU build: bytes taken off every launch's LDS request (the guard band's test)
#pragma once

#include <cstdlib>

// The variable as an integer (atoll of its text), dflt when it is not set.
inline long long kp_env_int(const char* name, long long dflt) {
  const char* v = getenv(name);
  return v ? atoll(v) : dflt;
}
// Whether the variable is set at all, whatever its value (KP_PAIR_ROWS=0 is on).
inline bool kp_env_flag(const char* name) { return getenv(name) != nullptr; }
