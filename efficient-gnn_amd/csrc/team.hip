// team.hip -- the value-free Chebyshev / Clenshaw step for VEC-4 signals as independent WAVES
// (reference calibration/WATS.py:32-36 recurrence, :65-68 heat sum by Clenshaw, :71-72
// normalisation fused into the last step).
//
// Why a second kernel.  cheb_step_kernel (step.hip) runs workgroup units of three kinds (team
// rows, a workgroup per long row, split-row chunks reduced through LDS) in one kernel: its
// register and scalar-register budget is the union of the three (106 SGPRs, 75 VGPRs: 6
// workgroups of 4 waves per CU), and a long row holds four waves until the slowest finishes.
// Here every wave is a unit of its own, described by one entry of a wave table built with the
// plan (build_team_waves):
//   * team waves: G / LN rows, LN sub-groups of LF lanes per row (LN | G = 64 / LF), the row's
//     4-entry chunks dealt to its sub-groups (ns, ns + LN, ...), summed by shuffles;
//   * part waves: one share of a long row (all G sub-groups on it); the wave writes its float64
//     partial with write-through (sc1) stores, drains them, and adds to the row's arrival
//     counter; the wave whose add completes the row sums every part's partial with sc1 loads in
//     part order and runs the epilogue (MI355X_MICROARCH.md, hand-off table row 1, as step.hip's
//     split rows, per wave instead of per workgroup).
// Every wave reads its column ids in SELL order (accumulate_sell: one coalesced id read per turn,
// pads are dropped loads), so the kernel has no LDS, no barrier and a lean register budget.
// The launches of a Clenshaw chain on u after its first run cheb_team4_spec_kernel, the same wave with
// the launch's mode fixed at compile time and its loads issued on one straight path (team_dev.h
// team_wave_spec, tuning key team_spec); every other launch runs cheb_team4_kernel.
#include <algorithm>
#include <cmath>
#include <vector>

#include "internal.h"

#include "team_dev.h"

namespace wg {
namespace {

template <int MINW, bool LATE, int CPT = 2>
__global__ __launch_bounds__(256, MINW) void cheb_team4_kernel(TeamArgs t) {
  const int w = (int)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (w < t.n_waves) team_wave<LATE, CPT>(t, w);
}

// the first launch of a folded chain (no permute-in pass): gathers of the caller's X0 scaled by
// dinv, the internal X0 written by the epilogues, and the closed-form rows after the table's waves
// GX: the gathers read the caller's X0 scaled by dinv (fold 1); else u_0 from a pass (fold 2)
template <bool GX>
__global__ __launch_bounds__(256, 6) void cheb_team4_first_kernel(TeamArgs t) {
  const int w = (int)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (w < t.n_waves) team_wave<false, 2, GX>(t, w);
  else if (w < t.n_waves + t.n_closed_waves) closed_wave(t, w - t.n_waves);
}

// the chain's launches after the first, one straight-line kernel per mode (team_dev.h team_wave_spec)
template <class M>
__global__ __launch_bounds__(256, 6) void cheb_team4_spec_kernel(TeamArgs t) {
  const int w = (int)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (w < t.n_waves) team_wave_spec<M>(t, w);
}

}  // namespace

void TeamPlan::release() {
  for (void* q : {(void*)wd, (void*)sell, (void*)wpart, (void*)warr, (void*)sell0, (void*)sdinv, (void*)ids16})
    (void)hipFree(q);
  *this = TeamPlan{};
}

// The first launch's id table (fold; plan_team_first): the SELL ids mapped to caller rows (perm) and
// each id slot's dinv
int build_team_first(wg_laplacian_s* L, TeamPlan* tp) {
  if (tp->sell0) return WG_OK;
  if (!tp->sell || tp->n_sell <= 0) return fail(WG_ERR_INVALID, "team first: no wave table");
  std::vector<int4> sell(tp->n_sell);
  WG_HIP_TRY(hipMemcpy(sell.data(), tp->sell, sizeof(int4) * sell.size(), hipMemcpyDeviceToHost));
  std::vector<int32_t> perm(L->n_rows);
  std::vector<double> dinv(L->n_cols);
  if (L->n_rows) WG_HIP_TRY(hipMemcpy(perm.data(), L->perm, sizeof(int32_t) * perm.size(), hipMemcpyDeviceToHost));
  if (L->n_cols) WG_HIP_TRY(hipMemcpy(dinv.data(), L->dinv, sizeof(double) * dinv.size(), hipMemcpyDeviceToHost));
  TeamFirstIds ids;
  int rc = plan_team_first(std::move(sell), perm, dinv, &ids);
  if (!rc) rc = upload(&tp->sell0, ids.sell0);
  if (!rc) rc = upload(&tp->sdinv, ids.sdinv);
  if (rc) free_all(tp->sell0, tp->sdinv);
  return rc;
}

// The wave table and SELL ids of the rows [0, n) of L's operator for LF-lane sub-groups
// (plan_team_waves), with the long rows' partials and arrival counters
// ids16: also the 16-bit ids of the waves' leading all-low turns (plan_team_ids16): only where the
// gathered columns are the rows' own numbering (no hybrid tail, shard or literal operator)
int build_team_waves(wg_laplacian_s* L, int64_t n, int LF, int iter, const int32_t* dcol,
                     const int32_t* drsplit, int order, bool ids16, TeamPlan* tp) {
  std::vector<int32_t> rs, col, re;  // the entries of row r are col[rs[r] .. re[r])
  if (int rc = download_csr(L, n, dcol, drsplit, &rs, &col, &re)) return rc;
  TeamWaves w;
  if (int rc = plan_team_waves(rs, re, col, LF, iter, order, &w)) return rc;
  TeamIds16 h;
  if (ids16)
    if (int rc = plan_team_ids16(&w, LF, &h)) return rc;
  if (h.ids.size() >= ((size_t)1 << 27)) return fail(WG_ERR_UNSUPPORTED, "team waves: 16-bit id array exceeds 2 GB");
  tp->n_ids16 = (int64_t)h.ids.size();
  tp->turns16 = h.turns16;
  tp->turns = 0;
  for (size_t i = 0; i < w.wd.size(); i += 2) tp->turns += w.wd[i].y >> 1;
  tp->max_parts = w.max_parts;
  tp->npot_rows = w.npot_rows;
  tp->n_waves = (int32_t)(w.wd.size() / 2);
  tp->n_sell = (int64_t)w.sell.size();
  tp->n_rows = n;
  tp->n_slots = w.n_slots;
  tp->n_long = w.n_long;
  tp->width = LF * 4;
  w.wd.resize(std::max<size_t>(w.wd.size(), 2), int4{0, 0, 0, 0});
  int rc = upload(&tp->wd, w.wd);
  if (!rc) rc = upload(&tp->sell, w.sell);
  if (!rc && !h.ids.empty()) rc = upload(&tp->ids16, h.ids);
  if (!rc) rc = dmalloc(&tp->wpart, (size_t)std::max(w.n_slots, 1) * tp->width);
  if (!rc) rc = dmalloc(&tp->warr, (size_t)std::max(w.n_long, 1));
  if (!rc && dzero(tp->warr, sizeof(uint32_t) * std::max(w.n_long, 1)) != hipSuccess)
    rc = fail(WG_ERR_HIP, "team waves: upload failed");
  if (rc) tp->release();  // no half-built table (wd non-null marks a built one)
  return rc;
}

int launch_team4(const TeamPlan& tp, const StepArgs& a, int variant, int spec, hipStream_t stream,
                 const TeamFirst* first) {
  TeamArgs t{};
  t.a = a;
  t.wd = tp.wd;
  t.n_waves = tp.n_waves;
  t.wpart = tp.wpart;
  t.warr = tp.warr;
  t.a.sell = tp.sell;
  t.ids16 = tp.ids16;
  team_args_debug(t, tp);
  if (first) {  // the folded chain's first launch
    const bool gx = first->gather_x0;
    if (gx && !tp.sell0) return fail(WG_ERR_INVALID, "launch_team4: no first-launch table");
    const int G = 64 / a.LF;
    t.a.first = 1;
    if (gx) {
      t.a.sell = tp.sell0;
      t.a.sdinv = tp.sdinv;
    }
    t.closed_from = first->closed_from;
    t.n_rows = first->n_rows;
    t.coef = first->coef;
    t.cS = first->S;
    t.cH = first->H;
    const int64_t nc = std::max<int64_t>(0, first->n_rows - first->closed_from);
    t.n_closed_waves = (int32_t)ceil_div(nc, (int64_t)G * kClosedRG);
    if (nc && (!t.cS || !t.cH)) return fail(WG_ERR_INVALID, "launch_team4: closed-form rows need S and H");
    const int64_t nw = (int64_t)tp.n_waves + t.n_closed_waves;
    if (nw <= 0) return WG_OK;
    if (gx) hipLaunchKernelGGL(cheb_team4_first_kernel<true>, dim3((unsigned)ceil_div(nw, 4)), dim3(256), 0, stream, t);
    else hipLaunchKernelGGL(cheb_team4_first_kernel<false>, dim3((unsigned)ceil_div(nw, 4)), dim3(256), 0, stream, t);
    WG_LAUNCH_CHECK();
    return WG_OK;
  }
  if (tp.n_waves <= 0) return WG_OK;
  const dim3 grid((unsigned)ceil_div(tp.n_waves, 4)), block(256);
  // the chain's own launches as straight-line kernels (tuning key team_spec); anything else generic
  const TeamMode mode = spec && variant == 1 ? team_mode_of(t.a) : kTeamGeneric;
  if (mode != kTeamGeneric) {
    if (mode == kTeamMid) hipLaunchKernelGGL(cheb_team4_spec_kernel<TeamMid>, grid, block, 0, stream, t);
    else if (mode == kTeamMidNoPrev) hipLaunchKernelGGL(cheb_team4_spec_kernel<TeamMidNoPrev>, grid, block, 0, stream, t);
    else hipLaunchKernelGGL(cheb_team4_spec_kernel<TeamFinal>, grid, block, 0, stream, t);
    WG_LAUNCH_CHECK();
    return WG_OK;
  }
  switch (variant) {
    case 7: hipLaunchKernelGGL((cheb_team4_kernel<7, false>), grid, block, 0, stream, t); break;
    case 8: hipLaunchKernelGGL((cheb_team4_kernel<8, false>), grid, block, 0, stream, t); break;
    case 9: hipLaunchKernelGGL((cheb_team4_kernel<8, true>), grid, block, 0, stream, t); break;
    case 10: hipLaunchKernelGGL((cheb_team4_kernel<6, true>), grid, block, 0, stream, t); break;
    case 11: hipLaunchKernelGGL((cheb_team4_kernel<6, false, 1>), grid, block, 0, stream, t); break;
    case 12: hipLaunchKernelGGL((cheb_team4_kernel<8, false, 1>), grid, block, 0, stream, t); break;
    case 13: hipLaunchKernelGGL((cheb_team4_kernel<8, true, 1>), grid, block, 0, stream, t); break;
    default: hipLaunchKernelGGL((cheb_team4_kernel<6, false>), grid, block, 0, stream, t);
  }
  WG_LAUNCH_CHECK();
  return WG_OK;
}

}  // namespace wg
