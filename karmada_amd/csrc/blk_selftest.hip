// blk_selftest.hip — test-only library (libkp_blktest.so): checks every GpuBlk
// primitive (kp_blk.h) on the device against a host computation, for several
// workgroup sizes and seeded random inputs; and runs the row-ranking kernel bodies of
// kp_kernels.h over caller-given rows; and runs webster_par (kp_select.h) over caller-given
// party lists at every block shape, reporting the exit each list took. Never linked into
// libkp.so.
#include <hip/hip_runtime.h>

#define KP_EXIT_MARKS 1  // kp_select.h: webster_par's exit marks (this library only)

#include <cstdio>
#include <cstring>
#include <vector>

#include "kp_blk.h"
#include "kp_pdq.h"
#include "kp_select.h"
#include "kp_kernels.h"

using namespace kp;

namespace {
// out layout per block: [0] sum64 [1] min64 [2] max64 [3] minu64 [4] and64 [5] or64
// [6] sum2.x [7] sum2.y [8] maxsum.max [9] maxsum.sum [10] any [11] bcast
// [12] andor.and [13] andor.or [14] scan total [15] find_bin bin [16] find_bin before
// [17] find_bin(rev) bin [18] find_bin(rev) before [19..19+nth) exclusive scan per thread
constexpr int kOut = 19;
}  // namespace

extern "C" __global__ void k_blk_test(const int64_t* in, const int32_t* cnt, int64_t kq, int64_t* out, int rounds) {
  extern __shared__ __align__(16) unsigned char smem[];
  GpuBlk B{(int64_t*)smem};
  uint32_t* hist = (uint32_t*)(smem + kRedBytes);
  const int t = B.tid();
  const int64_t v = in[blockIdx.x * B.nth() + t];
  int64_t* o = out + (size_t)blockIdx.x * (kOut + B.nth());
  // Repeat the sequence so that both scratch areas are reused many times.
  for (int r = 0; r < rounds; r++) {
    const int64_t s = B.sum64(v);
    const int64_t mn = B.min64(v);
    const int64_t mx = B.max64(v);
    const uint64_t mu = B.minu64((uint64_t)v);
    const uint64_t an = B.and64((uint64_t)v);
    const uint64_t on = B.or64((uint64_t)v);
    int64_t x = v, y = v ^ 0x5555;
    B.sum2(x, y);
    int64_t m2 = v, s2 = v >> 3;
    B.maxsum(m2, s2);
    const bool an1 = B.any(v == in[blockIdx.x * B.nth()] && t == B.nth() - 1);
    const int64_t bc = B.bcast(v * 3 + r);
    uint64_t a3 = (uint64_t)v, o3 = (uint64_t)v;
    B.andor(a3, o3);
    int32_t tot;
    const int32_t ex = B.excl_scan(cnt[blockIdx.x * B.nth() + t], &tot);
    for (int i = t; i < 256; i += B.nth()) hist[i] = 0;
    B.sync();
    atomicAdd(&hist[(uint64_t)v & 255], 1u);
    int64_t before, before2;
    const int bin = B.find_bin(hist, kq, &before, false);
    const int bin2 = B.find_bin(hist, kq, &before2, true);
    if (r == rounds - 1) {
      if (t == 0) {
        o[0] = s;
        o[1] = mn;
        o[2] = mx;
        o[3] = (int64_t)mu;
        o[4] = (int64_t)an;
        o[5] = (int64_t)on;
        o[6] = x;
        o[7] = y;
        o[8] = m2;
        o[9] = s2;
        o[10] = an1;
        o[11] = bc;
        o[12] = (int64_t)a3;
        o[13] = (int64_t)o3;
        o[14] = tot;
        o[15] = bin;
        o[16] = before;
        o[17] = bin2;
        o[18] = before2;
      }
      o[kOut + t] = ex;
    }
    B.sync();
  }
}

// Returns the number of mismatches (0 = pass); msg gets the first one.
extern "C" int kp_blk_selftest(int nth, int nblocks, uint64_t seed, char* msg, int msg_len) {
  const int n = nth * nblocks;
  std::vector<int64_t> in(n);
  std::vector<int32_t> cnt(n);
  uint64_t x = seed * 0x9E3779B97F4A7C15ull + 1;
  auto rnd = [&]() {
    x ^= x << 13;
    x ^= x >> 7;
    x ^= x << 17;
    return x;
  };
  for (int i = 0; i < n; i++) {
    const uint64_t r = rnd();
    switch (i % 4) {
      case 0: in[i] = (int64_t)r; break;
      case 1: in[i] = (int64_t)(r % 1000) - 500; break;
      case 2: in[i] = (int64_t)(r >> 20); break;
      default: in[i] = -(int64_t)(r >> 3); break;
    }
    cnt[i] = (int32_t)(rnd() % 7);
  }
  const int64_t kq = (int64_t)(rnd() % nth) + 1;
  int64_t *din, *dout;
  int32_t* dcnt;
  const size_t outn = (size_t)nblocks * (kOut + nth);
  if (hipMalloc(&din, 8 * n) || hipMalloc(&dcnt, 4 * n) || hipMalloc(&dout, 8 * outn)) {
    snprintf(msg, msg_len, "hipMalloc failed");
    return -1;
  }
  (void)hipMemcpy(din, in.data(), 8 * n, hipMemcpyHostToDevice);
  (void)hipMemcpy(dcnt, cnt.data(), 4 * n, hipMemcpyHostToDevice);
  hipLaunchKernelGGL(k_blk_test, dim3(nblocks), dim3(nth), kRedBytes + 1024, 0, din, dcnt, kq, dout, 5);
  if (hipDeviceSynchronize() != hipSuccess) {
    snprintf(msg, msg_len, "kernel failed: %s", hipGetErrorString(hipGetLastError()));
    return -1;
  }
  std::vector<int64_t> out(outn);
  (void)hipMemcpy(out.data(), dout, 8 * outn, hipMemcpyDeviceToHost);
  (void)hipFree(din);
  (void)hipFree(dcnt);
  (void)hipFree(dout);
  int bad = 0;
  auto check = [&](int blk, const char* what, int64_t got, int64_t want) {
    if (got != want) {
      if (!bad) snprintf(msg, msg_len, "nth=%d block %d %s: got %lld want %lld", nth, blk, what, (long long)got,
                         (long long)want);
      bad++;
    }
  };
  for (int b = 0; b < nblocks; b++) {
    const int64_t* v = in.data() + (size_t)b * nth;
    const int32_t* c = cnt.data() + (size_t)b * nth;
    const int64_t* o = out.data() + (size_t)b * (kOut + nth);
    int64_t s = 0, mn = INT64_MAX, mx = INT64_MIN, sy = 0, m2 = INT64_MIN, s2 = 0;
    uint64_t mu = ~0ull, an = ~0ull, on = 0;
    for (int i = 0; i < nth; i++) {
      s += v[i];
      mn = v[i] < mn ? v[i] : mn;
      mx = v[i] > mx ? v[i] : mx;
      mu = (uint64_t)v[i] < mu ? (uint64_t)v[i] : mu;
      an &= (uint64_t)v[i];
      on |= (uint64_t)v[i];
      sy += v[i] ^ 0x5555;
      m2 = v[i] > m2 ? v[i] : m2;
      s2 += v[i] >> 3;
    }
    check(b, "sum64", o[0], s);
    check(b, "min64", o[1], mn);
    check(b, "max64", o[2], mx);
    check(b, "minu64", o[3], (int64_t)mu);
    check(b, "and64", o[4], (int64_t)an);
    check(b, "or64", o[5], (int64_t)on);
    check(b, "sum2.x", o[6], s);
    check(b, "sum2.y", o[7], sy);
    check(b, "maxsum.max", o[8], m2);
    check(b, "maxsum.sum", o[9], s2);
    check(b, "any", o[10], v[nth - 1] == v[0] ? 1 : 0);
    check(b, "bcast", o[11], v[0] * 3 + 4);
    check(b, "andor.and", o[12], (int64_t)an);
    check(b, "andor.or", o[13], (int64_t)on);
    int64_t run = 0;
    for (int i = 0; i < nth; i++) {
      check(b, "excl_scan", o[kOut + i], run);
      run += c[i];
    }
    check(b, "scan total", o[14], run);
    int64_t h[256] = {0};
    for (int i = 0; i < nth; i++) h[(uint64_t)v[i] & 255]++;
    for (int rev = 0; rev < 2; rev++) {
      int64_t acc = 0;
      int bin = rev ? 0 : 255;
      int64_t before = 0;
      for (int q = 0; q < 256; q++) {
        const int idx = rev ? 255 - q : q;
        if (acc + h[idx] >= kq || q == 255) {
          bin = idx;
          before = acc;
          break;
        }
        acc += h[idx];
      }
      check(b, rev ? "find_bin(rev).bin" : "find_bin.bin", o[15 + 2 * rev], bin);
      check(b, rev ? "find_bin(rev).before" : "find_bin.before", o[16 + 2 * rev], before);
    }
  }
  return bad;
}

// ---------------------------------------------------------------------------
// sort.Sort wave emulation (kp_pdq.h) on the device: wave 0 of each block
// sorts its own list in LDS; the host compares with the serial emulation.
// ---------------------------------------------------------------------------
extern "C" __global__ void k_pdq_test(const int32_t* reps, const int32_t* offs, uint32_t* out_names,
                                      int32_t* out_ok) {
  extern __shared__ __align__(16) unsigned char smem[];
  GpuBlk B{(int64_t*)smem};
  const int a = offs[blockIdx.x], n = offs[blockIdx.x + 1] - a;
  PdqWave<GpuBlk> pw = pdq_carve(B, smem + kRedBytes, n);
  for (int i = B.tid(); i < n; i += B.nth()) {
    pw.name[i] = (uint32_t)i;
    pw.rep[i] = reps[a + i];
  }
  B.sync();
  int ok = 1;
  if (B.wid() == 0) ok = pw.run(n) ? 1 : 0;
  ok = B.bcast(ok);
  for (int i = B.tid(); i < n; i += B.nth()) out_names[a + i] = pw.name[i];
  if (B.tid() == 0) out_ok[blockIdx.x] = ok;
}

// Sorts nl lists (concatenated in reps, list j = [offs[j], offs[j+1])) on the
// device; out_names gets each list's permutation (indices into the list).
// Returns the number of lists the wave form declined, or -1 on a HIP error.
extern "C" int kp_pdq_selftest(const int32_t* reps, const int32_t* offs, int nl, int nth, uint32_t* out_names,
                               char* msg, int msg_len) {
  const int total = offs[nl];
  int maxn = 0;
  for (int j = 0; j < nl; j++) maxn = offs[j + 1] - offs[j] > maxn ? offs[j + 1] - offs[j] : maxn;
  int32_t *dr, *doffs, *dok;
  uint32_t* dn;
  if (hipMalloc(&dr, 4 * (size_t)(total + 1)) || hipMalloc(&doffs, 4 * (size_t)(nl + 1)) ||
      hipMalloc(&dn, 4 * (size_t)(total + 1)) || hipMalloc(&dok, 4 * (size_t)nl)) {
    snprintf(msg, msg_len, "hipMalloc failed");
    return -1;
  }
  (void)hipMemcpy(dr, reps, 4 * (size_t)total, hipMemcpyHostToDevice);
  (void)hipMemcpy(doffs, offs, 4 * (size_t)(nl + 1), hipMemcpyHostToDevice);
  const size_t smem = kRedBytes + pdq_wave_bytes(maxn);
  if (smem > 65536) (void)hipFuncSetAttribute((const void*)k_pdq_test, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
  hipLaunchKernelGGL(k_pdq_test, dim3(nl), dim3(nth), smem, 0, dr, doffs, dn, dok);
  if (hipDeviceSynchronize() != hipSuccess) {
    snprintf(msg, msg_len, "kernel failed: %s", hipGetErrorString(hipGetLastError()));
    return -1;
  }
  std::vector<int32_t> ok(nl);
  (void)hipMemcpy(out_names, dn, 4 * (size_t)total, hipMemcpyDeviceToHost);
  (void)hipMemcpy(ok.data(), dok, 4 * (size_t)nl, hipMemcpyDeviceToHost);
  (void)hipFree(dr);
  (void)hipFree(doffs);
  (void)hipFree(dn);
  (void)hipFree(dok);
  int declined = 0;
  for (int j = 0; j < nl; j++) declined += ok[j] ? 0 : 1;
  return declined;
}

// ---------------------------------------------------------------------------
// webster_reg (kp_select.h): Webster with one party per lane of one wave, in
// registers (k_select_top's subsets of <= 64 candidates). List j (at most 64 votes,
// party i = cluster rank i) with N[j] seats and the name order desc[j]; the host
// compares the seats with the oracle's AllocateWebsterSeats.
// ---------------------------------------------------------------------------
extern "C" __global__ void __launch_bounds__(64) k_webster_reg_test(const int64_t* votes, const int32_t* offs,
                                                                    const int32_t* Ns, const int32_t* descs,
                                                                    int32_t* seats, int32_t* ok) {
  extern __shared__ __align__(16) unsigned char smem[];
  WaveBlk B{(int64_t*)smem};
  const int a = offs[blockIdx.x], n = offs[blockIdx.x + 1] - a;
  const int l = B.lane();
  const bool has = l < n;
  const int64_t v = has ? votes[a + l] : 0;
  const int64_t V = B.sum64(v);
  bool okb = false;
  const WebRes w = webster_reg(B, has, (uint32_t)l, v, Ns[blockIdx.x], descs[blockIdx.x] != 0, V, &okb);
  if (has) seats[a + l] = web_seats(w, v, (uint32_t)l);
  if (l == 0) ok[blockIdx.x] = okb ? 1 : 0;
}

// Runs nl lists; seats_out gets every party's seats. Returns the number of lists
// webster_reg declined (its step bound), or -1 on a HIP error.
extern "C" int kp_webster_reg_selftest(const int64_t* votes, const int32_t* offs, const int32_t* Ns,
                                       const int32_t* descs, int nl, int32_t* seats_out, char* msg, int msg_len) {
  const int total = offs[nl];
  int64_t* dv;
  int32_t *doffs, *dN, *dd, *ds, *dok;
  if (hipMalloc(&dv, 8 * (size_t)(total + 1)) || hipMalloc(&doffs, 4 * (size_t)(nl + 1)) ||
      hipMalloc(&dN, 4 * (size_t)nl) || hipMalloc(&dd, 4 * (size_t)nl) || hipMalloc(&ds, 4 * (size_t)(total + 1)) ||
      hipMalloc(&dok, 4 * (size_t)nl)) {
    snprintf(msg, msg_len, "hipMalloc failed");
    return -1;
  }
  (void)hipMemcpy(dv, votes, 8 * (size_t)total, hipMemcpyHostToDevice);
  (void)hipMemcpy(doffs, offs, 4 * (size_t)(nl + 1), hipMemcpyHostToDevice);
  (void)hipMemcpy(dN, Ns, 4 * (size_t)nl, hipMemcpyHostToDevice);
  (void)hipMemcpy(dd, descs, 4 * (size_t)nl, hipMemcpyHostToDevice);
  hipLaunchKernelGGL(k_webster_reg_test, dim3(nl), dim3(64), 64, 0, dv, doffs, dN, dd, ds, dok);
  if (hipDeviceSynchronize() != hipSuccess) {
    snprintf(msg, msg_len, "kernel failed: %s", hipGetErrorString(hipGetLastError()));
    return -1;
  }
  std::vector<int32_t> ok(nl);
  (void)hipMemcpy(seats_out, ds, 4 * (size_t)total, hipMemcpyDeviceToHost);
  (void)hipMemcpy(ok.data(), dok, 4 * (size_t)nl, hipMemcpyDeviceToHost);
  (void)hipFree(dv);
  (void)hipFree(doffs);
  (void)hipFree(dN);
  (void)hipFree(dd);
  (void)hipFree(ds);
  (void)hipFree(dok);
  int declined = 0;
  for (int j = 0; j < nl; j++) declined += ok[j] ? 0 : 1;
  return declined;
}

// ---------------------------------------------------------------------------
// webster_par (kp_select.h), one block per list. List j = parties [offs[j], offs[j+1])
// with int32 votes in [0, 2^31) and a rank each, Ns[j] seats, the name order descs[j].
// SelScratch is laid out as carve_sel_scratch lays it out (whist 2 KB, hist 1 KB, buf)
// with `cap` entries of buf. pre != 0: the caller's first pass is done here and handed
// over as a WebPre (totals, the octave histogram in sc.hist, web_ctr zeroed), the
// contract of kp_paths.h; pre == 0: webster_par takes its own.
// Per party: web_seats. Per list: info[5] = mode, compact, np, Lb, exit marks (WebExit);
// and, when compact, the np entries of w.pl as (rank, seats) pairs in list order
// (pl_rank / pl_seats at [offs[j], offs[j] + np)), read after the return.
// ---------------------------------------------------------------------------
KP_HD inline size_t wpar_sel_bytes(int cap) { return 2048 + 1024 + 8 * (size_t)cap; }
template <class BLK>
KP_FI void body_webster_par_test(const BLK& B, unsigned char* sel, int cap, int pre, const int32_t* votes,
                                 const uint32_t* ranks, int n, int32_t N, bool desc, int32_t* seats,
                                 uint32_t* pl_rank, int32_t* pl_seats, int64_t* info) {
  SelScratch ss;
  ss.whist = (unsigned long long*)sel;
  ss.hist = (uint32_t*)(ss.whist + 256);
  ss.buf = (uint64_t*)(ss.hist + 256);
  ss.cap = cap;
  ss.dbg = (unsigned long long*)(info + 4);
  auto parties = [&](auto fn) {
    for (int i = B.tid(); i < n; i += B.nth()) fn(ranks[i], (int64_t)votes[i]);
  };
  WebPre wp{0, 0, 0};
  if (pre) {
    for (int i = B.tid(); i < 256; i += B.nth()) ss.hist[i] = 0;
    if (B.tid() == 0) *web_ctr(ss) = 0;
    B.sync();
    int64_t V = 0, vmax = 0, P = 0, none = 0;
    parties([&](uint32_t, int64_t v) {
      V += v;
      if (v > vmax) vmax = v;
      if (v > 0) {
        P++;
        kp_atomic_add(&ss.hist[vote_bin((uint32_t)v)], 1u);
      }
    });
    auto add = [](int64_t p, int64_t q) { return p + q; };
    B.reduce4(V, add, 0, P, add, 0, vmax, [](int64_t p, int64_t q) { return p > q ? p : q; }, INT64_MIN, none, add, 0);
    wp.V = V;
    wp.vmax = vmax;
    wp.P = P;
  }
  const WebRes w = webster_par(B, parties, N, desc, ss, pre ? &wp : nullptr);
  for (int i = B.tid(); i < n; i += B.nth()) seats[i] = web_seats(w, (int64_t)votes[i], ranks[i]);
  if (w.mode == 2 && w.compact)
    for (int i = B.tid(); i < w.np && i < n; i += B.nth()) {
      const uint64_t e = w.pl[i];
      pl_rank[i] = (uint32_t)(e >> 32);
      pl_seats[i] = web_seats(w, (int64_t)(uint32_t)e, (uint32_t)(e >> 32));
    }
  if (B.tid() == 0) {
    info[0] = w.mode;
    info[1] = w.compact ? 1 : 0;
    info[2] = w.np;
    info[3] = w.Lb;
  }
}

extern "C" __global__ void __launch_bounds__(1024) k_webster_par_test(int cap, int pre, const int32_t* votes,
                                                                      const uint32_t* ranks, const int32_t* offs,
                                                                      const int32_t* Ns, const int32_t* descs,
                                                                      int32_t* seats, uint32_t* pl_rank,
                                                                      int32_t* pl_seats, int64_t* info) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int j = (int)blockIdx.x, a = offs[j];
  body_webster_par_test(GpuBlk{(int64_t*)smem}, smem + kRedBytes, cap, pre, votes + a, ranks + a, offs[j + 1] - a,
                        Ns[j], descs[j] != 0, seats + a, pl_rank + a, pl_seats + a, info + 5 * (size_t)j);
}
// one wave alone on its list, as k_select_top's waves run webster_par
extern "C" __global__ void __launch_bounds__(64) k_webster_par_wave_test(int cap, int pre, const int32_t* votes,
                                                                         const uint32_t* ranks, const int32_t* offs,
                                                                         const int32_t* Ns, const int32_t* descs,
                                                                         int32_t* seats, uint32_t* pl_rank,
                                                                         int32_t* pl_seats, int64_t* info) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int j = (int)blockIdx.x, a = offs[j];
  body_webster_par_test(WaveBlk{(int64_t*)smem}, smem + 64, cap, pre, votes + a, ranks + a, offs[j + 1] - a, Ns[j],
                        descs[j] != 0, seats + a, pl_rank + a, pl_seats + a, info + 5 * (size_t)j);
}

// gpu: 0 the host block (CpuBlk), 1 GpuBlk with nth threads (64 .. 1024, a multiple of 64),
// 2 WaveBlk (one wave; nth ignored). seats_out / pl_rank / pl_seats: offs[nl] entries
// (pl_* are 0xFF.. / -1 where nothing was written); info: 5 int64 per list. Returns 0, or
// -1 with msg on a bad argument or a HIP error.
extern "C" int kp_webster_par_selftest(int gpu, int nth, int cap, int pre, const int32_t* votes, const uint32_t* ranks,
                                       const int32_t* offs, const int32_t* Ns, const int32_t* descs, int nl,
                                       int32_t* seats_out, uint32_t* pl_rank, int32_t* pl_seats, int64_t* info,
                                       char* msg, int msg_len) {
  const int total = offs[nl];
  if (cap < 0 || cap > 4096 || gpu < 0 || gpu > 2 || (gpu == 1 && (nth < 64 || nth > 1024 || nth % 64))) {
    snprintf(msg, msg_len, "bad argument: gpu=%d nth=%d cap=%d", gpu, nth, cap);
    return -1;
  }
  for (int j = 0; j < nl; j++)
    if (offs[j + 1] < offs[j]) {
      snprintf(msg, msg_len, "bad offsets at list %d", j);
      return -1;
    }
  memset(pl_rank, 0xFF, 4 * (size_t)total);
  memset(pl_seats, 0xFF, 4 * (size_t)total);
  memset(info, 0, 8 * 5 * (size_t)nl);
  if (!gpu) {
    std::vector<uint64_t> mem((kRedBytes + wpar_sel_bytes(cap)) / 8 + 1);
    unsigned char* sm = (unsigned char*)mem.data();
    for (int j = 0; j < nl; j++) {
      const int a = offs[j];
      body_webster_par_test(CpuBlk{(int64_t*)sm}, sm + kRedBytes, cap, pre, votes + a, ranks + a, offs[j + 1] - a, Ns[j],
                            descs[j] != 0, seats_out + a, pl_rank + a, pl_seats + a, info + 5 * (size_t)j);
    }
    return 0;
  }
  int32_t *dv, *doffs, *dN, *dd, *ds, *dps;
  uint32_t *dr, *dpr;
  int64_t* di;
  const size_t tb = 4 * (size_t)(total + 1);
  if (hipMalloc(&dv, tb) || hipMalloc(&dr, tb) || hipMalloc(&doffs, 4 * (size_t)(nl + 1)) ||
      hipMalloc(&dN, 4 * (size_t)nl + 4) || hipMalloc(&dd, 4 * (size_t)nl + 4) || hipMalloc(&ds, tb) ||
      hipMalloc(&dpr, tb) || hipMalloc(&dps, tb) || hipMalloc(&di, 8 * 5 * (size_t)nl + 8)) {
    snprintf(msg, msg_len, "hipMalloc failed");
    return -1;
  }
  (void)hipMemcpy(dv, votes, 4 * (size_t)total, hipMemcpyHostToDevice);
  (void)hipMemcpy(dr, ranks, 4 * (size_t)total, hipMemcpyHostToDevice);
  (void)hipMemcpy(doffs, offs, 4 * (size_t)(nl + 1), hipMemcpyHostToDevice);
  (void)hipMemcpy(dN, Ns, 4 * (size_t)nl, hipMemcpyHostToDevice);
  (void)hipMemcpy(dd, descs, 4 * (size_t)nl, hipMemcpyHostToDevice);
  (void)hipMemset(ds, 0xFF, tb);
  (void)hipMemset(dpr, 0xFF, tb);
  (void)hipMemset(dps, 0xFF, tb);
  (void)hipMemset(di, 0, 8 * 5 * (size_t)nl + 8);
  const size_t smem = (gpu == 1 ? kRedBytes : 64) + wpar_sel_bytes(cap);
  int rc = 0;
  if (nl > 0) {
    if (gpu == 1) {
      if (smem > 65536)
        (void)hipFuncSetAttribute((const void*)k_webster_par_test, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
      hipLaunchKernelGGL(k_webster_par_test, dim3(nl), dim3(nth), smem, 0, cap, pre, dv, dr, doffs, dN, dd, ds, dpr, dps,
                         di);
    } else {
      if (smem > 65536)
        (void)hipFuncSetAttribute((const void*)k_webster_par_wave_test, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)smem);
      hipLaunchKernelGGL(k_webster_par_wave_test, dim3(nl), dim3(64), smem, 0, cap, pre, dv, dr, doffs, dN, dd, ds, dpr,
                         dps, di);
    }
  }
  if (hipDeviceSynchronize() != hipSuccess) {
    snprintf(msg, msg_len, "kernel failed: %s", hipGetErrorString(hipGetLastError()));
    rc = -1;
  } else {
    (void)hipMemcpy(seats_out, ds, 4 * (size_t)total, hipMemcpyDeviceToHost);
    (void)hipMemcpy(pl_rank, dpr, 4 * (size_t)total, hipMemcpyDeviceToHost);
    (void)hipMemcpy(pl_seats, dps, 4 * (size_t)total, hipMemcpyDeviceToHost);
    (void)hipMemcpy(info, di, 8 * 5 * (size_t)nl, hipMemcpyDeviceToHost);
  }
  (void)hipFree(dv);
  (void)hipFree(dr);
  (void)hipFree(doffs);
  (void)hipFree(dN);
  (void)hipFree(dd);
  (void)hipFree(ds);
  (void)hipFree(dpr);
  (void)hipFree(dps);
  (void)hipFree(di);
  return rc;
}

// The two row-ranking kernels of kp_schedule_affinities_ex (kp_kernels.h body_est_rows_rank,
// body_flt_rows_rank) over caller-given rows and permutation, with the launch shapes of
// kernels.hip (gpu != 0) or on the host block (gpu == 0): est_src[n_est][C] ->
// est_dst[n_est][Cp], flt_src[n_flt][ceil(C/64)] -> flt_dst[n_flt][Cp/64]; perm has Cp
// entries. Returns 0, or -1 on a HIP error.
extern "C" __global__ void __launch_bounds__(256) k_est_rows_rank_test(int C, int Cp, const uint32_t* perm,
                                                                     const int32_t* src, int32_t* dst) {
  body_est_rows_rank(GpuBlk{nullptr}, (int)blockIdx.x, C, Cp, perm, src, dst);
}
extern "C" __global__ void __launch_bounds__(256) k_flt_rows_rank_test(int n_rows, int C, int W, const uint32_t* perm,
                                                                     const uint64_t* src, uint64_t* dst) {
  const int i = (int)(blockIdx.x * 4) + kp_uniform((int)(threadIdx.x >> 6));
  if (i >= n_rows * W) return;
  body_flt_rows_rank(GpuBlk{nullptr}, i / W, i % W, C, W, perm, src, dst);
}

extern "C" int kp_rows_rank_selftest(int gpu, int C, int Cp, const uint32_t* perm, const int32_t* est_src, int n_est,
                                     int32_t* est_dst, const uint64_t* flt_src, int n_flt, uint64_t* flt_dst,
                                     char* msg, int msg_len) {
  const int W = Cp / 64, Wc = (C + 63) / 64;
  if (!gpu) {
    for (int r = 0; r < n_est; r++) body_est_rows_rank(CpuBlk{nullptr}, r, C, Cp, perm, est_src, est_dst);
    for (int i = 0; i < n_flt * W; i++) body_flt_rows_rank(CpuBlk{nullptr}, i / W, i % W, C, W, perm, flt_src, flt_dst);
    return 0;
  }
  uint32_t* dp;
  int32_t *des, *ded;
  uint64_t *dfs, *dfd;
  const size_t es = 4 * (size_t)n_est * C, ed = 4 * (size_t)n_est * Cp, fs = 8 * (size_t)n_flt * Wc,
               fd = 8 * (size_t)n_flt * W;
  if (hipMalloc(&dp, 4 * (size_t)Cp) || hipMalloc(&des, es + 4) || hipMalloc(&ded, ed + 4) || hipMalloc(&dfs, fs + 8) ||
      hipMalloc(&dfd, fd + 8)) {
    snprintf(msg, msg_len, "hipMalloc failed");
    return -1;
  }
  (void)hipMemcpy(dp, perm, 4 * (size_t)Cp, hipMemcpyHostToDevice);
  (void)hipMemcpy(des, est_src, es, hipMemcpyHostToDevice);
  (void)hipMemcpy(dfs, flt_src, fs, hipMemcpyHostToDevice);
  (void)hipMemset(ded, 0xA5, ed);
  (void)hipMemset(dfd, 0xA5, fd);
  if (n_est > 0) hipLaunchKernelGGL(k_est_rows_rank_test, dim3(n_est), dim3(256), 0, 0, C, Cp, dp, des, ded);
  if (n_flt > 0 && W > 0)
    hipLaunchKernelGGL(k_flt_rows_rank_test, dim3((n_flt * W + 3) / 4), dim3(256), 0, 0, n_flt, C, W, dp, dfs, dfd);
  int rc = 0;
  if (hipDeviceSynchronize() != hipSuccess) {
    snprintf(msg, msg_len, "kernel failed: %s", hipGetErrorString(hipGetLastError()));
    rc = -1;
  } else {
    (void)hipMemcpy(est_dst, ded, ed, hipMemcpyDeviceToHost);
    (void)hipMemcpy(flt_dst, dfd, fd, hipMemcpyDeviceToHost);
  }
  (void)hipFree(dp);
  (void)hipFree(des);
  (void)hipFree(ded);
  (void)hipFree(dfs);
  (void)hipFree(dfd);
  return rc;
}
