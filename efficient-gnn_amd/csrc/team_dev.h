// team_dev.h -- the independent-wave unit of the value-free step (team.hip), shared with the
// hybrid step's fused launch (tiles.hip hybrid_fused_kernel): the wave table's descriptors, the
// closed-form rows of a folded chain's first launch, and one wave's rows.
#pragma once

#include "step_dev.h"

namespace wg {
namespace {

// wave descriptor (two int4 per wave):
//   d0 = {first SELL chunk, chunks per sub-group, first row, LN | rows << 8 | part << 16 | n16 << 17}
//        (n16: leading turns also held as 16-bit ids, plan_host.h TeamIds16; team_wave_spec alone reads it)
//   d1 = {part index, parts of the row, first partial slot, arrival counter}   (part waves only)
struct TeamArgs {
  StepArgs a;
  const int4* wd;
  const int4* ids16;  // the 16-bit ids of turns [0, n16) of each wave (null: every n16 is 0)
  int32_t n_waves;
  double* wpart;   // [slots][LF * 4] float64 partials of part waves
  uint32_t* warr;  // [long rows] arrival counters (0 between launches: the last arrival resets)
  // the first launch of a folded chain (a.first) also finishes the purely isolated rows [closed_from,
  // n_rows) in closed form, S = coef * X0 and H = S / (|S|_1 + 1e-8) at their caller rows (what the
  // permute-in pass did), in n_closed_waves extra waves after the table's
  int32_t n_closed_waves;
  int64_t closed_from, n_rows;
  double coef;
  float* cS;
  float* cH;
#ifdef WG_DEBUG_BOUNDS
  int64_t dbg_rows, dbg_slots, dbg_long;  // the table's rows, partial slots and long rows
#endif
};

// the debug variant's plan sizes (WG_DEBUG_BOUNDS; nothing in the shipped library)
inline void team_args_debug(TeamArgs& t, const TeamPlan& tp) {
#ifdef WG_DEBUG_BOUNDS
  t.dbg_rows = tp.n_rows;
  t.dbg_slots = tp.n_slots;
  t.dbg_long = tp.n_long;
  t.a.dbg_sell_bytes = 16ull * (uint64_t)tp.n_sell;
#else
  (void)t;
  (void)tp;
#endif
}

constexpr int kClosedRG = 4;  // row groups per closed-form wave (their loads all issued before any use)

// rows [closed_from, n_rows): one LF-lane sub-group per row, kClosedRG groups of G rows per wave
__device__ __forceinline__ void closed_wave(const TeamArgs& t, int64_t cw) {
  const StepArgs& a = t.a;
  const int lane = threadIdx.x & 63;
  const int LF = a.LF;
  const int G = 64 / LF;
  const int sg = lane / LF;
  const int fs = lane - sg * LF;
  int64_t rows[kClosedRG], rs[kClosedRG];
  bool act[kClosedRG];
  float x[kClosedRG][4];
#pragma unroll
  for (int q = 0; q < kClosedRG; ++q) {
    rows[q] = t.closed_from + (cw * kClosedRG + q) * G + sg;
    act[q] = sg < G && rows[q] < t.n_rows;
    rs[q] = act[q] ? a.perm_in[rows[q]] : 0;
  }
#pragma unroll
  for (int q = 0; q < kClosedRG; ++q)
    if (act[q]) load_vec<4>(a.x0c + rs[q] * a.ld + fs * 4, x[q]);
#pragma unroll
  for (int q = 0; q < kClosedRG; ++q) {
    double sv[4];
    double part = 0.0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      sv[j] = stored(t.coef * (double)x[q][j]);
      part += fabs(sv[j]);
    }
    double tot = 0.0;  // the row's L1 norm, in column order (finalize_kernel's order)
    for (int r = 0; r < LF; ++r) tot += __shfl(part, sg * LF + r, 64);
    if (!act[q]) continue;
    const double den = tot + 1e-8;
    double h[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) h[j] = sv[j] / den;
    store_vec<4>(t.cS + rs[q] * a.ld + fs * 4, sv);
    store_vec<4>(t.cH + rs[q] * a.ld + fs * 4, h);
  }
}

// MINW: minimum waves per SIMD the registers are held to (6 = the natural 77 VGPRs); LATE: the
// epilogue's X0 / previous-row operands loaded after the gathers instead of before (fewer live
// registers in the loop)
template <bool LATE, int CPT, bool FIRST = false>
__device__ __forceinline__ void team_wave(const TeamArgs& t, int w) {
  const StepArgs& a = t.a;
#ifdef WG_TIMING_PROBES
  if (a.probe_h2 == -4) return;  // launch + wave dispatch only
#endif
  int4 d0 = t.wd[2 * w];  // uniform address: a scalar load
  const int lane = threadIdx.x & 63;
  const int LF = a.LF;
  const int G = 64 / LF;
  const int sg = lane / LF;
  const int fs = lane - sg * LF;
  const int LN = d0.w & 0xff;
  const int tpw = (d0.w >> 8) & 0xff;
  const bool part = (d0.w >> 16) & 1;
  const int team = sg / LN;
  const int ns = sg - team * LN;
  const int64_t row = (int64_t)d0.z + team;
  const bool active = sg < G && team < tpw;
  WG_DCHECK(d0.z >= 0 && (int64_t)d0.z + (part ? 1 : tpw) <= t.dbg_rows && d0.y >= 0 && LN >= 1 && (part || tpw * LN <= G),
            "wave %d: descriptor {%d, %d, %d, %#x} outside the %lld-row table", w, d0.x, d0.y, d0.z, d0.w,
            (long long)t.dbg_rows);
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  EpiIn<4> in;
#ifdef WG_TIMING_PROBES
  if (a.probe_h2 == -3) {  // no ids, gathers or epilogue operands: one 16-B store per row
    if (active && ns == 0 && a.xk)
      *reinterpret_cast<float4*>(a.xk + row * a.ld + fs * 4) = float4{0.f, 0.f, 0.f, 0.f};
    return;
  }
  if (a.probe_h2 == -2) d0.y = 0;  // no ids, no gathers
#endif
  if (active) {
    if (!LATE && ns == 0 && !part && !a.tsum) epi_prefetch<4>(a, row, fs, in);
    accumulate_sell<CPT, FIRST>(a, int2{d0.x, d0.y}, G, sg, fs, acc);
    if (LATE && ns == 0 && !part && !a.tsum) epi_prefetch<4>(a, row, fs, in);
  }
  reduce_subgroups<4>(acc, LN, LF, team * LN * LF, fs);  // every lane (shuffles)
  bool emit = active && ns == 0;
  int lane0 = team * LN * LF;
  if (part) {  // a share of a long row: float64 partial (sc1), drained, then one arrival per wave
    const int4 d1 = t.wd[2 * w + 1];
    const int width = LF * 4;
    WG_DCHECK(d1.x >= 0 && d1.x < d1.y && d1.z >= 0 && (int64_t)d1.z + d1.y <= t.dbg_slots && d1.w >= 0 &&
                  d1.w < t.dbg_long,
              "part wave %d: {%d, %d, %d, %d} outside %lld slots / %lld long rows", w, d1.x, d1.y, d1.z, d1.w,
              (long long)t.dbg_slots, (long long)t.dbg_long);
    if (lane < LF) {
      double* p = t.wpart + (int64_t)(d1.z + d1.x) * width + lane * 4;
#pragma unroll
      for (int j = 0; j < 4; ++j) __hip_atomic_store(p + j, acc[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    int last = 0;
    if (lane == 0) {
      // the arrival that completes the row resets its counter: every launch starts from 0, whatever
      // the history of earlier launches (uint32, compared for equality: no wrap-around modulus)
      const uint32_t old = __hip_atomic_fetch_add(t.warr + d1.w, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      last = old + 1u == (uint32_t)d1.y;
      if (last) __hip_atomic_store(t.warr + d1.w, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    last = __shfl(last, 0, 64);
    if (!last || lane >= LF) return;
    // the last arriver: lanes 0 .. LF-1 (sub-group 0: fs == lane) sum every part's partial in
    // part order (deterministic) and share the team rows' epilogue below (one inlined copy)
    if (!a.tsum) epi_prefetch<4>(a, row, lane, in);
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = 0.0;
    for (int q = 0; q < d1.y; ++q) {
      const double* p = t.wpart + (int64_t)(d1.z + q) * width + lane * 4;
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[j] += __hip_atomic_load(p + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    emit = true;
    lane0 = 0;
  }
  if (emit) {
    if (a.tsum) {  // the row's sums only (hybrid_epilogue_kernel adds the dense blocks and finishes the row)
      double* p = a.tsum + row * a.ld + fs * 4;
      *reinterpret_cast<double2*>(p) = double2{acc[0], acc[1]};
      *reinterpret_cast<double2*>(p + 2) = double2{acc[2], acc[3]};
      return;
    }
    part_add<4>(a, row, fs, acc);
    step_epilogue<4>(a, row, fs, acc, in, lane0);
  }
}

// ---- the chain's own launches as straight-line kernels (tuning key team_spec) ----
//
// The Clenshaw chain on u (capi.hip wavelet_chain) makes, after its folded first launch, three kinds
// of launch.  A mode fixes every launch-uniform flag of one kind at compile time (team_mode_of picks
// it from StepArgs; any other combination, the first launch included, runs team_wave): clen, uin = 1,
// x0 and iso present, k = 2, the sc1 T_k store (nt 8), no tsum / phase / probe / out-of-table checks.
//   kClen   1 = a step (u_k stored with sc1), 2 = the final step (S and H at caller rows out_perm)
//   kPrev   xm2 present and holding u (uprev)
struct TeamMid { static constexpr int kClen = 1; static constexpr bool kPrev = true; };
struct TeamMidNoPrev { static constexpr int kClen = 1; static constexpr bool kPrev = false; };
struct TeamFinal { static constexpr int kClen = 2; static constexpr bool kPrev = true; };

enum TeamMode { kTeamGeneric = 0, kTeamMid, kTeamMidNoPrev, kTeamFinal };

inline TeamMode team_mode_of(const StepArgs& a) {
#if defined(WG_TIMING_PROBES) || defined(WG_DEBUG_BOUNDS)
  (void)a;
  return kTeamGeneric;
#else
  if (!a.clen || !a.uin || a.val || a.k != 2 || a.first || a.tsum || a.phase || a.probe || (a.nt & 12) != 8 ||
      !a.x0 || !a.iso || !a.dinv || !a.sell)
    return kTeamGeneric;
  const bool prev = a.xm2 != nullptr;
  if (prev != (a.uprev != 0)) return kTeamGeneric;
  if (a.clen == 1 && a.uout && a.xk) return prev ? kTeamMid : kTeamMidNoPrev;
  if (a.clen == 2 && !a.uout && !a.xk && prev && a.S && a.H && a.out_perm && a.S_out) return kTeamFinal;
  return kTeamGeneric;
#endif
}

// a row's epilogue operands as loaded registers (raw bits; masked lanes hold 0)
struct EpiRegs {
  u32x4_t prev, x0;
  uint32_t dlo, dhi;  // dinv (float64)
  uint32_t iso;
  uint32_t orow;      // the final step: out_perm[row]
};

// every lane issues the loads, lanes with `on` false past the buffers' ends (no request); nothing here
// waits
template <class M>
__device__ __forceinline__ void epi_issue(const StepArgs& a, int row, int fs, bool on, EpiRegs& in) {
  const uint32_t r = (uint32_t)row;
  const uint32_t off = on ? r * ((uint32_t)a.ld * 4u) + (uint32_t)fs * 16u : kOobOff;
  in.orow = 0;
  if constexpr (M::kClen == 2)
    in.orow = __builtin_amdgcn_raw_buffer_load_b32(buf_of(a.out_perm, 0x7fffffffu), on ? r * 4u : kOobOff, 0, 0);
  in.iso = __builtin_amdgcn_raw_buffer_load_b8(buf_of(a.iso, 0x7fffffffu), on ? r : kOobOff, 0, 0);
  const u32x2_t d = __builtin_amdgcn_raw_buffer_load_b64(buf_of(a.dinv, 0x7fffffffu), on ? r * 8u : kOobOff, 0, 0);
  in.dlo = d.x;
  in.dhi = d.y;
  if constexpr (M::kPrev) in.prev = __builtin_amdgcn_raw_buffer_load_b128(buf_of(a.xm2, a.u_bytes), off, 0, 0);
  else in.prev = u32x4_t{0u, 0u, 0u, 0u};
  in.x0 = __builtin_amdgcn_raw_buffer_load_b128(buf_of(a.x0, a.u_bytes), off, 0, 0);
}

// step_epilogue's arithmetic for one mode, operation for operation as the generic kernel compiles it
// (contraction off and the fused operations written out, so S and H keep their bits):
//   acc *= -dinv;  isolated row: acc = fma(-1/dinv, u_own, acc)
//   t = fma(-1/dinv, prev, fma(ck, X0, cacc * acc));  u = t * dinv
// rinv: 1 / dinv (kPrev modes; the others divide in the isolated row's branch)
template <class M>
__device__ __forceinline__ void epilogue_spec(const StepArgs& a, int row, int fs, double (&acc)[4],
                                              const EpiRegs& in, double rinv, int lane0) {
#pragma clang fp contract(off)
  const int64_t off = (int64_t)row * a.ld + (int64_t)fs * 4;
  const double dinv = __hiloint2double((int)in.dhi, (int)in.dlo);
  const float x0[4] = {__uint_as_float(in.x0.x), __uint_as_float(in.x0.y), __uint_as_float(in.x0.z),
                       __uint_as_float(in.x0.w)};
  const float prev[4] = {__uint_as_float(in.prev.x), __uint_as_float(in.prev.y), __uint_as_float(in.prev.z),
                         __uint_as_float(in.prev.w)};
#pragma unroll
  for (int j = 0; j < 4; ++j) acc[j] = acc[j] * -dinv;
  if (in.iso) {  // L_hat_ii = -1: the own row of u, as b
    float x[4];
    load_vec<4>(a.xm1 + off, x);
    const double xs = M::kPrev ? rinv : 1.0 / dinv;
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = fma(-xs, (double)x[j], acc[j]);
  }
  double t[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    t[j] = fma(a.ck, (double)x0[j], a.cacc * acc[j]);
    if constexpr (M::kPrev) t[j] = fma(-rinv, (double)prev[j], t[j]);
  }
  if constexpr (M::kClen == 1) {
    double u[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) u[j] = t[j] * dinv;
    store_vec_sc1<4>(a.xk + off, u);
  } else {  // the final step: S = t and H = S / (|S|_1 + 1e-8) at the caller's row
    const int64_t oo = (int64_t)(int32_t)in.orow * a.ld + (int64_t)fs * 4;
    store_vec<4>(a.S_out + oo, t);
    double part = 0.0;
#pragma unroll
    for (int j = 0; j < 4; ++j) part += fabs(stored(t[j]));
    double tot = 0.0;
    for (int q = 0; q < a.LF; ++q) tot += __shfl(part, lane0 + q, 64);
    const double den = tot + 1e-8;
    double h[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) h[j] = stored(t[j]) / den;
    store_vec<4>(a.H + oo, h);
  }
}

// team_wave for one chain mode.  Issue order: descriptor; the first turn's ids; the row's epilogue
// operands (all in flight together; vmcnt retires in order, so the ids go first and the first wait is
// the one the gathers need); the gather loop, a step's 1 / dinv computed behind the first turn's
// gathers; the epilogue.  A long row's last arriver issues its first four parts' partials, then the
// operands, before the first add (part order kept).
// H16: the wave's first n16 >= 1 turns are on 16-bit ids (one chunk per turn: accumulate_sell16_from).
// The two forms are whole paths of their own from the descriptor to the stores (team_wave_spec picks one
// per wave), so no loaded register of one meets the other's at a join.
template <class M, bool H16>
__device__ __forceinline__ void team_wave_spec_on(const TeamArgs& t, int w, const int4 d0) {
  const StepArgs& a = t.a;
  const int lane = threadIdx.x & 63;
  const int LF = a.LF;
  const int G = 64 / LF;
  const int sg = lane / LF;
  const int fs = lane - sg * LF;
  const int LN = d0.w & 0xff;
  const int tpw = (d0.w >> 8) & 0xff;
  const bool part = (d0.w >> 16) & 1;
  const int team = sg / LN;
  const int ns = sg - team * LN;
  const int row = d0.z + team;  // rows are 24-bit ids (gather4_applies)
  const bool active = sg < G && team < tpw;
  const int ny = d0.y;
  const int n16 = (int)((uint32_t)d0.w >> kIds16Shift);  // leading turns on 16-bit ids (2 n16 <= ny)
  const uint32_t cstep = (uint32_t)G * 16u;
  const uint32_t off0 = ((uint32_t)d0.x + (uint32_t)sg) * 16u;
  const uint32_t off16 = (ids16_base((uint32_t)d0.x) + (uint32_t)sg) * 16u;
  const __amdgpu_buffer_rsrc_t ri = buf_of(a.sell, 0x7fffffffu);
  u32x4_t h0 = {0u, 0u, 0u, 0u}, c0 = h0, c1 = h0;  // (a single-chunk wave does not read c1)
  if constexpr (H16) {
    h0 = __builtin_amdgcn_raw_buffer_load_b128(buf_of(t.ids16, 0x7fffffffu), active ? off16 : kOobOff, 0, (int)(1u << 31));
  } else {
    c0 = __builtin_amdgcn_raw_buffer_load_b128(ri, active && ny > 0 ? off0 : kOobOff, 0, (int)(1u << 31));
    if (ny > 1) c1 = __builtin_amdgcn_raw_buffer_load_b128(ri, active ? off0 + cstep : kOobOff, 0, (int)(1u << 31));
  }
  EpiRegs in;
  const bool own = active && ns == 0 && !part;
  epi_issue<M>(a, row, fs, own, in);
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  double rinv = 0.0;
  // 1 / dinv where it is placed, not hoisted in front of the gathers (dinv itself goes through the
  // empty asm, so no second copy of it stays live)
  auto divide = [&](EpiRegs& e) {
    asm volatile("" : "+v"(e.dlo), "+v"(e.dhi));
    return 1.0 / __hiloint2double((int)e.dhi, (int)e.dlo);
  };
  // behind the first turn's gathers: a step's 1 / dinv (the final launch has no registers to hold it
  // across the loop within 80)
  // (nor has the 16-bit path of a step: there the division goes behind the loop too)
  constexpr bool kDivEarly = M::kPrev && M::kClen == 1 && !H16;
  auto behind = [&] {
    if constexpr (kDivEarly) rinv = divide(in);
  };
  const uint32_t off32 = off0 + (uint32_t)(2 * n16) * cstep;  // the chunks behind the 16-bit turns
  if constexpr (H16)
    accumulate_sell16_from(a, t.ids16, h0, off16, n16, c0, c1, off32, ny - 2 * n16, cstep, fs, active, acc, behind);
  accumulate_sell_from<!H16>(a, c0, c1, off32, cstep, ny - 2 * n16, fs, active, acc, !H16, behind);  // every lane
  if (ny <= 0) behind();  // no turn to hide it behind
  if constexpr (M::kPrev && !kDivEarly) rinv = divide(in);
  reduce_subgroups<4>(acc, LN, LF, team * LN * LF, fs);  // every lane (shuffles)
  if (!part) {
    if (own) epilogue_spec<M>(a, row, fs, acc, in, rinv, team * LN * LF);
    return;
  }
  {  // a share of a long row: float64 partial (sc1), drained, then one arrival per wave
    const int4 d1 = t.wd[2 * w + 1];
    const int width = LF * 4;
    if (lane < LF) {
      double* p = t.wpart + (int64_t)(d1.z + d1.x) * width + lane * 4;
#pragma unroll
      for (int j = 0; j < 4; ++j) __hip_atomic_store(p + j, acc[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    int last = 0;
    if (lane == 0) {  // the arrival that completes the row resets its counter (team_wave)
      const uint32_t old = __hip_atomic_fetch_add(t.warr + d1.w, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      last = old + 1u == (uint32_t)d1.y;
      if (last) __hip_atomic_store(t.warr + d1.w, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    last = __shfl(last, 0, 64);
    if (!last || lane >= LF) return;
    // the last arriver: lanes 0 .. LF-1 (fs == lane).  The row's partial slots as one raw buffer that
    // ends with the row's last part: the first four parts are loaded whole before the first add
    // (write-through sc1 loads, 32 B per lane and part), parts past the last return 0.0, and a sum that
    // started from +0.0 is never -0.0, so adding that 0.0 leaves it as it is
    const __amdgpu_buffer_rsrc_t rp = buf_of(t.wpart + (int64_t)d1.z * width, (uint32_t)d1.y * (uint32_t)width * 8u);
    constexpr int kSc1Volatile = 16 | (int)(1u << 31);
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    auto load_part = [&](int q, u32x4_t& lo, u32x4_t& hi) {
      const uint32_t o = (uint32_t)q * (uint32_t)width * 8u + (uint32_t)lane * 32u;
      lo = __builtin_amdgcn_raw_buffer_load_b128(rp, o, 0, kSc1Volatile);
      hi = __builtin_amdgcn_raw_buffer_load_b128(rp, o + 16u, 0, kSc1Volatile);
    };
    auto add_part = [&](const u32x4_t& lo, const u32x4_t& hi) {
      s[0] += __hiloint2double((int)lo.y, (int)lo.x);
      s[1] += __hiloint2double((int)lo.w, (int)lo.z);
      s[2] += __hiloint2double((int)hi.y, (int)hi.x);
      s[3] += __hiloint2double((int)hi.w, (int)hi.z);
    };
    u32x4_t plo[4], phi[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) load_part(u, plo[u], phi[u]);
    EpiRegs lin;  // the operands with the first batch, behind it (the sums do not wait for them)
    epi_issue<M>(a, row, lane, true, lin);
#pragma unroll
    for (int u = 0; u < 4; ++u) add_part(plo[u], phi[u]);
    for (int q0 = 4; q0 < d1.y; q0 += 2) {  // rows of more than four parts: two at a time
      load_part(q0, plo[0], phi[0]);
      load_part(q0 + 1, plo[1], phi[1]);
      add_part(plo[0], phi[0]);
      add_part(plo[1], phi[1]);
    }
    epilogue_spec<M>(a, row, lane, s, lin, M::kPrev ? divide(lin) : 0.0, 0);
  }
}

template <class M>
__device__ __forceinline__ void team_wave_spec(const TeamArgs& t, int w) {
  const int4 d0 = t.wd[2 * w];  // uniform address: a scalar load
  if (((uint32_t)d0.w >> kIds16Shift) > 0) team_wave_spec_on<M, true>(t, w, d0);
  else team_wave_spec_on<M, false>(t, w, d0);
}

}  // namespace
}  // namespace wg
