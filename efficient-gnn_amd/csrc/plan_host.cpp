// plan_host.cpp -- the host-side planners of the step kernels' tables: pure functions from the host
// CSR and a few knobs to vectors (plan_host.h).  The wave, part and chunk orders written here fix the
// kernels' summation order.  No HIP call: checked under ASan / UBSan by tests/c/plan_check.cpp.
#include "plan_host.h"

#include <algorithm>
#include <climits>
#include <cstdio>
#include <utility>

namespace wg {

// The first launch's id table (fold): the SELL ids mapped to caller rows (perm) and each id slot's
// dinv (float64; 0 for pads, whose gathers return 0)
int plan_team_first(std::vector<int4> sell_in, const std::vector<int32_t>& perm, const std::vector<double>& dinv,
                    TeamFirstIds* out) {
  const int64_t n_rows = (int64_t)perm.size();
  std::vector<int4>& sell = out->sell0;
  sell = std::move(sell_in);  // mapped in place
  std::vector<double>& sd = out->sdinv;
  sd.assign(sell.size() * 4, 0.0);
  for (size_t i = 0; i < sell.size(); ++i) {
    int32_t* id = &sell[i].x;
    for (int j = 0; j < 4; ++j) {
      if (id[j] == kPadCol) continue;
      if (id[j] < 0 || id[j] >= n_rows || (size_t)id[j] >= dinv.size())
        return fail(WG_ERR_INVALID, "team first: column %d outside the rows", id[j]);
      sd[4 * i + j] = dinv[id[j]];
      id[j] = perm[id[j]];
    }
  }
  return WG_OK;
}

// The wave table and SELL ids of the rows [0, n) of an operator (internal order, rows by
// descending length) for LF-lane sub-groups: a row of nch 4-entry chunks gets LN sub-groups, the
// smallest divisor of G with ceil(nch / LN) <= tch chunks each (tch = iter / 4, even); consecutive
// rows with the same LN share a wave (G / LN rows); a row longer than G * tch chunks is dealt to
// ceil(nch / (G * tch)) part waves.  Every sub-group of a wave runs the wave's chunk count (two chunks per turn, a single one last when it is odd),
// shorter ones padded with kPadCol chunks.
int plan_team_waves(const std::vector<int32_t>& rs, const std::vector<int32_t>& re, const std::vector<int32_t>& col,
                    int LF, int iter, int order, TeamWaves* out) {
  if (rs.empty() || re.size() + 1 != rs.size() || LF < 1 || LF > 64 || order < 0 || order > 7)
    return fail(WG_ERR_INVALID, "team waves: %zu row starts, %zu row ends, LF %d, order %d", rs.size(), re.size(), LF,
                order);
  const int64_t n = (int64_t)re.size();
  const int G = 64 / LF;
  const int64_t tch = std::max<int64_t>(2, (iter / 4 + 1) / 2 * 2);
  auto rlen = [&](int64_t r) -> int64_t { return re[r] - rs[r]; };
  std::vector<int> divs;
  for (int d = 1; d <= G; ++d)
    if (G % d == 0) divs.push_back(d);
  std::vector<int4>& wd = out->wd;
  std::vector<int4>& sell = out->sell;
  wd.clear();
  sell.clear();
  const int4 pad4{kPadCol, kPadCol, kPadCol, kPadCol};
  int32_t slots = 0, longs = 0;
  out->max_parts = out->npot_rows = 0;
  auto chunk = [&](int64_t r, int64_t ch) {  // the 4 ids of chunk ch of row r
    int32_t id[4];
    for (int i = 0; i < 4; ++i) {
      const int64_t e = (int64_t)rs[r] + ch * 4 + i;
      id[i] = e < re[r] ? col[e] : kPadCol;
    }
    return int4{id[0], id[1], id[2], id[3]};
  };
  auto fits = [&]() {
    return sell.size() < ((size_t)1 << 27);  // 16-B chunks at 32-bit byte offsets (accumulate_sell)
  };
  int64_t r = 0;
  while (r < n) {
    const int64_t nch0 = (rlen(r) + 3) / 4;
    if (nch0 > (int64_t)G * tch) {  // a long row: part waves, all G sub-groups on one share each
      const int64_t per = (int64_t)G * tch;
      const int32_t parts = (int32_t)((nch0 + per - 1) / per);
      for (int32_t q = 0; q < parts; ++q) {
        const int64_t c0 = q * per, c1 = std::min<int64_t>(nch0, c0 + per);
        const int64_t nchs = (c1 - c0 + G - 1) / G;  // chunks per sub-group
        wd.push_back(int4{(int32_t)sell.size(), (int32_t)nchs, (int32_t)r, G | (1 << 8) | (1 << 16)});
        wd.push_back(int4{q, parts, slots, longs});
        const size_t base = sell.size();
        sell.resize(base + (size_t)nchs * G, pad4);
        for (int64_t c = c0; c < c1; ++c) sell[base + (size_t)(c - c0)] = chunk(r, c);  // chunk k: k / G, k % G
        if (!fits()) return fail(WG_ERR_UNSUPPORTED, "team waves: id array exceeds 2 GB");
      }
      slots += parts;
      ++longs;
      out->max_parts = std::max(out->max_parts, parts);
      if (parts & (parts - 1)) ++out->npot_rows;
      ++r;
      continue;
    }
    int LN = G;
    for (int d : divs)
      if ((nch0 + d - 1) / d <= tch) {
        LN = d;
        break;
      }
    const int tpw = G / LN;
    int rows = 0;
    while (rows < tpw && r + rows < n) {  // consecutive rows with the same LN
      const int64_t nch = (rlen(r + rows) + 3) / 4;
      if (nch > (int64_t)G * tch) break;
      int ln = G;
      for (int d : divs)
        if ((nch + d - 1) / d <= tch) {
          ln = d;
          break;
        }
      if (ln != LN) break;
      ++rows;
    }
    int64_t nchs = 0;  // chunks per sub-group: the wave's most (sub-group 0 of its longest row)
    for (int i = 0; i < rows; ++i) {
      const int64_t nch = (rlen(r + i) + 3) / 4;
      nchs = std::max<int64_t>(nchs, (nch + LN - 1) / LN);
    }
    wd.push_back(int4{(int32_t)sell.size(), (int32_t)nchs, (int32_t)r, LN | (rows << 8)});
    wd.push_back(int4{0, 0, 0, 0});
    const size_t base = sell.size();
    sell.resize(base + (size_t)nchs * G, pad4);
    for (int i = 0; i < rows; ++i) {
      const int64_t nch = (rlen(r + i) + 3) / 4;
      for (int ns = 0; ns < LN; ++ns)
        for (int64_t k = 0; ns + k * LN < nch; ++k)
          sell[base + (size_t)k * G + (size_t)(i * LN + ns)] = chunk(r + i, ns + k * LN);
    }
    if (!fits()) return fail(WG_ERR_UNSUPPORTED, "team waves: id array exceeds 2 GB");
    r += rows;
  }
  sell.resize(sell.size() + (size_t)4 * G, pad4);  // the next-turn id reads past the last wave
  if (order) {  // dispatch order of the waves (the table is built longest rows first)
    const size_t nw = wd.size() / 2;
    std::vector<int4> o;
    o.reserve(wd.size());
    // 1: reversed (shortest rows first); 2 ..: fa waves from the longest end, then fb from the
    // shortest, repeated.  2 (one and one) mixes long and short rows in every workgroup: arxiv
    // F = 40 33.9 vs 34.7 us; whole workgroups alternating (7) put every long row on every other
    // XCD (round-robin placement): 51.9 (r04 s28)
    static const int kFa[8] = {0, 0, 1, 2, 4, 1, 1, 4}, kFb[8] = {0, 0, 1, 1, 1, 2, 4, 4};
    size_t lo = 0, hi = nw;
    while (lo < hi) {
      if (order == 1) {
        --hi;
        o.push_back(wd[2 * hi]);
        o.push_back(wd[2 * hi + 1]);
        continue;
      }
      for (int q = 0; q < kFa[order] && lo < hi; ++q, ++lo) {
        o.push_back(wd[2 * lo]);
        o.push_back(wd[2 * lo + 1]);
      }
      for (int q = 0; q < kFb[order] && lo < hi; ++q) {
        --hi;
        o.push_back(wd[2 * hi]);
        o.push_back(wd[2 * hi + 1]);
      }
    }
    wd.swap(o);
  }
  out->n_slots = slots;
  out->n_long = longs;
  return WG_OK;
}

// 16-bit ids of the waves' leading all-low full turns (plan_host.h TeamIds16): columns are sorted in a
// row and rows numbered by descending length, so the ids past 65534 are a row's last entries and a
// wave's leading turns are low
int plan_team_ids16(TeamWaves* w, int LF, TeamIds16* out) {
  if (LF < 1 || LF > 64 || (w->wd.size() & 1)) return fail(WG_ERR_INVALID, "team ids16: LF %d, %zu descriptors", LF, w->wd.size());
  const size_t G = (size_t)(64 / LF);
  const std::vector<int4>& sell = w->sell;
  out->ids.clear();
  out->turns16 = out->turns = 0;
  auto low = [](const int4& c) {
    const int32_t* id = &c.x;
    for (int i = 0; i < 4; ++i)
      if (id[i] != kPadCol && (id[i] < 0 || id[i] >= (int32_t)kIds16Pad)) return false;
    return true;
  };
  auto half = [](int32_t id) -> uint32_t { return id == kPadCol ? kIds16Pad : (uint32_t)id; };
  auto pack = [&](const int4& a, const int4& b) {
    return int4{(int32_t)(half(a.x) | half(a.y) << 16), (int32_t)(half(a.z) | half(a.w) << 16),
                (int32_t)(half(b.x) | half(b.y) << 16), (int32_t)(half(b.z) | half(b.w) << 16)};
  };
  for (size_t i = 0; i < w->wd.size(); i += 2) {
    int4& d0 = w->wd[i];
    if (d0.x < 0 || d0.y < 0 || (size_t)d0.x + (size_t)d0.y * G > sell.size() || ((uint32_t)d0.w >> kIds16Shift))
      return fail(WG_ERR_INVALID, "team ids16: wave %zu: descriptor {%d, %d, %d, %#x}", i / 2, d0.x, d0.y, d0.z, d0.w);
    const size_t x = (size_t)d0.x;
    const int full = std::min(d0.y >> 1, kIds16Max);
    int n16 = 0;
    for (; n16 < full; ++n16) {
      bool ok = true;
      for (size_t c = x + 2 * (size_t)n16 * G; ok && c < x + 2 * (size_t)(n16 + 1) * G; ++c) ok = low(sell[c]);
      if (!ok) break;
    }
    out->turns += d0.y >> 1;
    out->turns16 += n16;
    if (!n16) continue;
    if (out->ids.empty()) out->ids.assign((sell.size() + 1) / 2, int4{-1, -1, -1, -1});
    const size_t b = ids16_base((uint32_t)x);
    for (size_t t = 0; t < (size_t)n16; ++t)
      for (size_t sg = 0; sg < G; ++sg)
        out->ids[b + t * G + sg] = pack(sell[x + 2 * t * G + sg], sell[x + (2 * t + 1) * G + sg]);
    d0.w |= (int32_t)((uint32_t)n16 << kIds16Shift);
  }
  return WG_OK;
}

// smallest divisor of G that is >= want (G itself if none smaller)
int divisor_at_least(int G, int64_t want) {
  for (int d = 1; d <= G; ++d)
    if (G % d == 0 && d >= want) return d;
  return G;
}

// Defaults measured on MI355X (profiles/r01 sweeps): wide signals (G = 64/LF
// small, e.g. F = 40 -> G = 6) want long per-sub-group runs; F = 1 (G = 64)
// shorter ones.
// Wide tiles (F >= 16) on large graphs: one sub-group per row up to 192 entries per
// lane (ogbn-arxiv-size F=40: 41.8 vs 45.5 us per step with iter 96 vs 24; F=64 56.3
// vs 64.9; Reddit-size F=44 1732 vs 1817 us; with the value-free Clenshaw chain,
// s47-s49: 192 vs 96 -- arxiv F=40 37.3 vs 38.2, F=64 49.9 vs 51.8, Reddit-size F=44
// 1497 vs 1522; 256 jumps to 55 us) and long split-row chunks (Reddit-size
// F=44: 1625 us with chunk_iter 128 vs 1729 with 64) above 16 M nonzeros, 64 below
// (arxiv F=40 36.5 vs 37.1 us, F=64 neutral; profiles/r01/s55_chunk_sweep.log); small graphs
// keep more lanes per row for latency (PubMed-size F=40: 9.3 us with iter 24, 17.2
// with 96).  F = 1 from 1 M nonzeros: 8 entries per lane (ogbn-arxiv-size: 10.7 us per
// step vs 11.6 with 16, s34).
// t_*: the tuning keys (0 = the shape-dependent default)
void default_knobs(int t_iter, int t_block_iter, int t_chunk_iter, int G, int64_t nnz, int* iter, int* block_iter,
                   int* chunk_iter, bool hybrid, int64_t rows) {
  // the hybrid step's tail (~22 % of each row's entries) wants longer one-row
  // sub-groups and larger block / split units the more rows there are to fill the CUs with
  // (Reddit-size F=41, rows / (G x 256 CUs): 182 -> iter 6144: 784 vs 917 us per step with the
  // gather kernel's defaults; its 2-way shards (92) -> 1536: 415 vs 473; the 4-way shards (46)
  // keep the defaults: 1536 gives 232-234 vs 246-249 on three ranks but 312 vs 247 on the fourth
  // (a long-tailed row walked by one sub-group), the 8-way shards (23) 172 vs 156;
  // profiles/r02/s72-s76).  Only from 8 M nonzeros: on the arxiv-size graph (2.3 M, hub rows of
  // thousands of tail entries walked by one sub-group) the 1536 tier took 67.8 vs 38.6 us
  // (profiles/r03/s20-s21)
  const int64_t per_cu = rows / ((int64_t)G * 256);
  if (hybrid && per_cu >= 64 && nnz >= ((int64_t)8 << 20)) {
    const bool big = per_cu >= 128;
    *iter = t_iter > 0 ? t_iter : (big ? 6144 : 1536);
    *block_iter = t_block_iter > 0 ? t_block_iter : (big ? 4096 : 1024);
    *chunk_iter = t_chunk_iter > 0 ? t_chunk_iter : (big ? 4096 : 1024);
    return;
  }
  const bool wide = G <= 16;
  const bool big = nnz >= (int64_t)1 << 20;
  // from 8 M nonzeros: longer team runs and 256-iteration split-row chunks (Reddit-size F=41,
  // width 48: 1400 vs 1434 us per step; its 8-way shard, 14.3 M nonzeros: 195-200 vs 207-211
  // with the 1-16 M defaults, profiles/r02/s39-s40)
  const bool large = nnz >= (int64_t)1 << 23;
  *iter = t_iter > 0 ? t_iter : (wide ? (large ? 384 : big ? 192 : 24) : (G == 64 && big ? 8 : 16));
  *block_iter = t_block_iter > 0 ? t_block_iter : (wide ? 256 : 32);
  *chunk_iter = t_chunk_iter > 0 ? t_chunk_iter : (wide ? (large ? 256 : big ? 64 : 32) : 16);
}

int64_t count_split_rows(const SegKnobs& k, const unsigned int* bucket) {
  if (!k.reordered) return 0;
  const int64_t block_max = (int64_t)k.NW * k.G * k.block_iter;
  int64_t n_split = 0;
  for (int b = kBuckets - 1; b >= 0; --b) {
    const int64_t maxlen = (b == 0) ? 1 : (1ll << b);
    if (maxlen > block_max) n_split += bucket[b];
  }
  return n_split;
}

// The segment table and the split-row chunk table.
//   team  rows: len <= G*iter              (LN sub-groups per row, LN | G)
//   block rows: len <= 4G*block_iter       (one workgroup per row)
//   split rows: longer                     (one workgroup per CH = 4G*chunk_iter nnz + combine_kernel)
// Classification is by power-of-two length bucket (rows are sorted by length).
int plan_segments(const SegKnobs& kn, int64_t n, const unsigned int* bucket, const std::vector<int32_t>& rp,
                  SegPlan* out) {
  const int G = kn.G, NW = kn.NW, iter = kn.iter, block_iter = kn.block_iter, chunk_iter = kn.chunk_iter;
  if (G < 1 || NW < 1 || iter < 1 || block_iter < 1 || chunk_iter < 1 || n < 0)
    return fail(WG_ERR_INVALID, "segments: G %d, %d waves, knobs %d / %d / %d", G, NW, iter, block_iter, chunk_iter);
  const int64_t base = 0;  // first row of the plan
  const int64_t team_max = (int64_t)G * iter;
  const int64_t block_max = (int64_t)NW * G * block_iter;
  const int64_t CH = (int64_t)NW * G * chunk_iter;
  *out = SegPlan{};
  SegTable& t = out->tab;
  char buf[256];
  if (!kn.reordered) {
    // caller order: a single team segment sized by the average row length
    const int ln = divisor_at_least(G, ceil_div(std::max<int64_t>(1, kn.avg_len), iter));
    const int tpw = G / ln;
    t.s[0] = Seg{0, (int32_t)n, 0, ln, 0};
    t.n = n > 0 ? 1 : 0;
    t.total_blocks = (int32_t)ceil_div(n, NW * tpw);
    snprintf(buf, sizeof(buf), "team rows[0,%lld) ln=%d (no reorder)\n", (long long)n, ln);
    out->text = buf;
    return WG_OK;
  }
  int64_t n_split = 0, n_block = 0;
  for (int b = kBuckets - 1; b >= 0; --b) {
    const int64_t maxlen = (b == 0) ? 1 : (1ll << b);
    if (maxlen > block_max) n_split += bucket[b];
    else if (maxlen > team_max) n_block += bucket[b];
  }
  int nseg = 0;
  int32_t blk = 0;
  if (n_split > 0) {
    if ((int64_t)rp.size() < n_split + 1)
      return fail(WG_ERR_INVALID, "segments: %zu row starts for %lld split rows", rp.size(), (long long)n_split);
    std::vector<ChunkDesc>& ch = out->chunks;
    std::vector<int2>& rc = out->rowchunks;
    rc.resize(n_split);
    for (int64_t r = 0; r < n_split; ++r) {
      const int64_t len = rp[r + 1] - rp[r];
      const int cnt = (int)std::max<int64_t>(1, ceil_div(len, CH));
      rc[r] = make_int2((int)ch.size(), cnt);
      for (int q = 0; q < cnt; ++q) {
        ChunkDesc d{};
        d.row = (int32_t)(base + r);
        d.e0 = (int32_t)(rp[r] + q * CH);
        d.e1 = (int32_t)std::min<int64_t>(rp[r + 1], rp[r] + (q + 1) * CH);
        ch.push_back(d);
      }
    }
    const int32_t n_chunks = (int32_t)ch.size();
    out->n_split = (int32_t)n_split;
    t.s[nseg++] = Seg{0, n_chunks, 0, G, 2};
    blk = n_chunks;
    snprintf(buf, sizeof(buf), "split rows[%lld,%lld) chunks=%d CH=%lld (+combine)\n", (long long)base,
             (long long)(base + n_split), n_chunks, (long long)CH);
    out->text += buf;
  }
  if (n_block > 0) {
    t.s[nseg++] = Seg{(int32_t)(base + n_split), (int32_t)(base + n_split + n_block), blk, G, 1};
    blk += (int32_t)n_block;
    snprintf(buf, sizeof(buf), "block rows[%lld,%lld) (workgroup per row)\n", (long long)(base + n_split),
             (long long)(base + n_split + n_block));
    out->text += buf;
  }
  int32_t row = (int32_t)(base + n_split + n_block);
  const int first_team = nseg;
  for (int b = kBuckets - 1; b >= 0; --b) {
    const int32_t cnt = (int32_t)bucket[b];
    const int64_t maxlen = (b == 0) ? 1 : (1ll << b);
    if (!cnt || maxlen > team_max) continue;
    int ln = divisor_at_least(G, ceil_div(maxlen, iter));
    Seg* last = nseg > first_team ? &t.s[nseg - 1] : nullptr;
    if (last && (last->ln == ln || nseg == kMaxSeg)) {
      if (last->ln != ln) ln = last->ln;  // out of slots: extend
      last->end = row + cnt;
      blk = last->blk_begin + (int32_t)ceil_div(last->end - last->begin, NW * (G / ln));
    } else {
      t.s[nseg++] = Seg{row, row + cnt, blk, ln, 0};
      blk += (int32_t)ceil_div(cnt, NW * (G / ln));
    }
    row += cnt;
  }
  t.n = nseg;
  t.total_blocks = blk;
  for (int i = first_team; i < nseg; ++i) {
    snprintf(buf, sizeof(buf), "team rows[%d,%d) ln=%d blocks=%d\n", t.s[i].begin, t.s[i].end, t.s[i].ln,
             (i + 1 < nseg ? t.s[i + 1].blk_begin : blk) - t.s[i].blk_begin);
    out->text += buf;
  }
  return WG_OK;
}

// The padded CSR of the value-free VEC-4 gathers (accumulate_u4): every row's column ids padded
// to a multiple of 4 with kPadCol, row pointers prp, kPcolTail pad ids after the last row.
int plan_pcol(const std::vector<int32_t>& rp, const std::vector<int32_t>& col, PaddedCsr* out) {
  if (rp.empty()) return fail(WG_ERR_INVALID, "build_pcol: no row starts");
  const int64_t n = (int64_t)rp.size() - 1;
  std::vector<int32_t>& prp = out->prp;
  prp.assign(n + 1, 0);
  prp[0] = 0;
  for (int64_t r = 0; r < n; ++r) {
    const int64_t len = rp[r + 1] - rp[r];
    const int64_t padded = prp[r] + (len + 3) / 4 * 4;
    if (padded > INT32_MAX - kPcolTail) return fail(WG_ERR_INVALID, "build_pcol: padded CSR exceeds int32");
    prp[r + 1] = (int32_t)padded;
  }
  std::vector<int32_t>& pc = out->pcol;
  pc.assign((size_t)prp[n] + kPcolTail, kPadCol);
  for (int64_t r = 0; r < n; ++r)
    std::copy(col.begin() + rp[r], col.begin() + rp[r + 1], pc.begin() + prp[r]);
  return WG_OK;
}

// The SELL order of a plan's value-free team waves (accumulate_sell): for wave w = unit * NW + wave
// of a team segment, sub-group g (row begin + (unit - blk_begin) NW tpw + wave tpw + g / LN, share
// ns = g % LN of the row's 4-entry chunks: ns, ns + LN, ...), its k-th chunk at
// sell[wmeta[w].x + k G + g] with k = 2 t + c; every sub-group padded with kPadCol chunks to the
// wave's turn count wmeta[w].y (2 chunks per turn), plus 2 turns of pads after the last wave.
int plan_sell(const SegTable& tab, int NW, int LF, const std::vector<int32_t>& rp, const std::vector<int32_t>& col,
              SellTable* out) {
  if (LF < 1 || LF > 64 || NW < 1 || tab.n < 0 || tab.n > kMaxSeg || tab.total_blocks < 0)
    return fail(WG_ERR_INVALID, "build_sell: LF %d, %d waves, %d segments", LF, NW, tab.n);
  const int G = 64 / LF;
  std::vector<int2>& wm = out->wmeta;
  wm.assign((size_t)tab.total_blocks * NW, int2{0, 0});
  std::vector<int4>& sell = out->sell;
  sell.clear();
  const int4 pad4{kPadCol, kPadCol, kPadCol, kPadCol};
  for (int si = 0; si < tab.n; ++si) {
    const Seg& sg = tab.s[si];
    if (sg.mode != 0) continue;
    if (sg.ln < 1 || G % sg.ln || sg.begin < 0 || sg.end < sg.begin || (size_t)sg.end + 1 > rp.size())
      return fail(WG_ERR_INVALID, "build_sell: segment %d rows [%d, %d) ln %d", si, sg.begin, sg.end, sg.ln);
    const int LN = sg.ln, tpw = G / LN;
    const int32_t nblk = (si + 1 < tab.n ? tab.s[si + 1].blk_begin : tab.total_blocks) - sg.blk_begin;
    for (int32_t u = 0; u < nblk; ++u) {
      for (int w = 0; w < NW; ++w) {
        const int64_t r0 = (int64_t)sg.begin + (int64_t)u * NW * tpw + (int64_t)w * tpw;
        int64_t turns = 0;
        for (int g = 0; g < G; ++g) {  // the wave's longest sub-group
          const int64_t r = r0 + g / LN, ns = g % LN;
          if (g / LN >= tpw || r >= sg.end) continue;
          const int64_t nch = (rp[r + 1] - rp[r] + 3) / 4;
          const int64_t mine = ns < nch ? (nch - ns + LN - 1) / LN : 0;
          turns = std::max<int64_t>(turns, (mine + 1) / 2);
        }
        const size_t wi = (size_t)(sg.blk_begin + u) * NW + w;
        if (sell.size() + (size_t)(2 * G * (turns + 2)) >= ((size_t)1 << 27))  // 16-B chunks at 32-bit byte offsets
          return fail(WG_ERR_UNSUPPORTED, "build_sell: id array exceeds 2 GB (tuning key sell = 0)");
        wm[wi] = int2{(int)sell.size(), (int)(2 * turns)};  // chunk count (accumulate_sell)
        const size_t base = sell.size();
        sell.resize(base + (size_t)2 * turns * G, pad4);
        for (int g = 0; g < G; ++g) {
          const int64_t r = r0 + g / LN, ns = g % LN;
          if (g / LN >= tpw || r >= sg.end) continue;
          const int64_t len = rp[r + 1] - rp[r];
          const int64_t nch = (len + 3) / 4;
          for (int64_t k = 0; ns + k * LN < nch; ++k) {
            const int64_t ch = ns + k * LN;
            int32_t id[4];
            for (int i = 0; i < 4; ++i) id[i] = ch * 4 + i < len ? col[rp[r] + ch * 4 + i] : kPadCol;
            sell[base + (size_t)k * G + g] = int4{id[0], id[1], id[2], id[3]};
          }
        }
      }
    }
  }
  sell.resize(sell.size() + (size_t)4 * G, pad4);  // the next-turn id reads past the last wave
  return WG_OK;
}

// The hybrid step's plan of rows [0, n_plan) of the n = rp.size() - 1 rows: each (row block, column
// tile) pair holding at least th entries is a dense block (bct, row masks bmask); the rest of each
// row (its tail) comes first in the row's range of tcol, up to tsplit[r]
int plan_tiles(const std::vector<int32_t>& rp, const std::vector<int32_t>& col, int64_t n_plan, int64_t n_cols,
               int64_t col_limit, const TileKnobs& kn, TileTables* out) {
  if (rp.empty() || n_plan < 0 || n_plan > (int64_t)rp.size() - 1 || col_limit > n_cols || kn.th < 1 ||
      (kn.rows != 64 && kn.rows != 128) || (int64_t)col.size() < rp.back())
    return fail(WG_ERR_INVALID, "tiles: %lld of %zu rows, column limit %lld of %lld, th %d, %d-row blocks",
                (long long)n_plan, rp.size(), (long long)col_limit, (long long)n_cols, kn.th, kn.rows);
  const int64_t n = (int64_t)rp.size() - 1, nnz = (int64_t)col.size();
  const int th = kn.th;
  const int tmax = kn.tile_max;  // <= 0: auto (below)
  const int kTR = kn.rows;
  *out = TileTables{};
  const int64_t n_ct = ceil_div(n_cols, kTC);
  std::vector<int32_t> cnt(n_ct, 0), sel(n_ct, -1), touched, tmp;
  std::vector<int32_t>& bct = out->bct;
  std::vector<int32_t>& tcol = out->tcol;
  std::vector<int32_t>& tsplit = out->tsplit;
  tcol = col;
  tsplit.assign(n, 0);
  std::vector<uint32_t>& bmask = out->bmask;
  std::vector<int4>& items = out->items;
  std::vector<int4>& multi = out->multi;
  std::vector<int2> rbs;  // row blocks with dense blocks: {row block, first block}
  int64_t dense = 0;
  for (int64_t r = n_plan; r < n; ++r) tsplit[r] = rp[r + 1];  // unplanned rows: all tail
  const int64_t n_rb = ceil_div(n_plan, kTR);
  for (int64_t rb = 0; rb < n_rb; ++rb) {
    const int64_t r0 = rb * kTR, r1 = std::min<int64_t>(r0 + kTR, n_plan);
    touched.clear();
    for (int64_t r = r0; r < r1; ++r)
      for (int32_t e = rp[r]; e < rp[r + 1]; ++e) {
        const int32_t c = col[e];
        if (c < 0 || c >= col_limit) return fail(WG_ERR_INVALID, "tiles: column %d of row %lld outside [0, %lld)", c,
                                                 (long long)r, (long long)col_limit);
        if (cnt[c / kTC]++ == 0) touched.push_back(c / kTC);
      }
    std::sort(touched.begin(), touched.end());
    const int32_t first = (int32_t)bct.size();
    for (int32_t ct : touched)
      if (cnt[ct] >= th) {
        sel[ct] = (int32_t)bct.size();
        bct.push_back(ct);
      }
    bmask.resize(bct.size() * kTR, 0u);
    for (int64_t r = r0; r < r1; ++r) {
      tmp.clear();
      for (int32_t e = rp[r]; e < rp[r + 1]; ++e) {
        const int32_t c = col[e];
        const int32_t s = sel[c / kTC];
        if (s >= 0) {
          uint32_t& w = bmask[(size_t)s * kTR + (r - r0)];
          const uint32_t bit = 1u << (c % kTC);
          if (w & bit) {  // a repeated entry: a row mask cannot count it twice -- keep the gather kernel
            *out = TileTables{};
            return WG_OK;
          }
          w |= bit;
          ++dense;
        } else {
          tmp.push_back(c);
        }
      }
      if (kn.probe_tailwin > 0) {  // timing probe only (results wrong): every tail column folded
        const int64_t win = std::max<int64_t>(1, col_limit / kn.probe_tailwin);  // into one window
        for (auto& c : tmp) c = (int32_t)(col_limit / 2 + c % win < col_limit ? col_limit / 2 + c % win : c % win);
      }
      tsplit[r] = rp[r] + (int32_t)tmp.size();
      std::copy(tmp.begin(), tmp.end(), tcol.begin() + rp[r]);
    }
    for (int32_t ct : touched) {
      cnt[ct] = 0;
      sel[ct] = -1;
    }
    const int32_t nb = (int32_t)bct.size() - first;
    if (nb > 0) rbs.push_back(make_int2((int)rb, first));  // nb == 0: every entry is tail, no part added
  }
  // work items: a row block's dense blocks, split over several workgroups (slots) past tmax, one list
  // per form (the plan serves every width; hybrid_fused_shape picks the form per width at launch).  Auto
  // (tile_max <= 0) for the sequential and two-stream steps: 128 blocks per workgroup from 100 k rows, else 64
  // (Reddit-size F=41, width 48, us per step: whole graph 726 at 128 vs 735 at 192, 2-way shard 369 vs
  // 382; smaller shards want more workgroups, profiles/r02/s80-s81).  Where the fused launch takes the
  // plan (hybrid_fused_kernel: the tail's waves fill the GPU beside the items) fewer, longer items pay,
  // about n_plan / 310 blocks each: 8-way shard 101.6 at 96 vs 103.9 at 64 and 103.0 at 112, 4-way 173
  // at 128-192 vs 212.8 at 64 and 196 at 256, 2-way 326-331 at 384 vs 340 at 320 and 368-371 at 512,
  // whole graph 692-694 at 640-768 vs 705 at 512 and 745 at 1024 (r05 s55-s65)
  const int64_t nblk = (int64_t)bct.size();
  // one item list per form: {items, multi, slots}
  auto make_items = [&](int tm, std::vector<int4>& its, std::vector<int4>& mul) {
    tm = std::max(1, std::min(tm, kItemMax));
    int32_t ns = 0;
    for (size_t q0 = 0; q0 < rbs.size(); ++q0) {
      const int rb = rbs[q0].x, first = rbs[q0].y;
      const int32_t nb = (int32_t)((q0 + 1 < rbs.size() ? rbs[q0 + 1].y : nblk) - first);
      const int32_t k = (nb + tm - 1) / tm;
      if (k == 1) {
        its.push_back(make_int4(rb, first, first + nb, -1));
      } else {
        for (int32_t q = 0; q < k; ++q)
          its.push_back(make_int4(rb, first + (int32_t)((int64_t)nb * q / k), first + (int32_t)((int64_t)nb * (q + 1) / k),
                                  ns + q));
        mul.push_back(make_int4(rb, ns, k, 0));
        ns += k;
      }
    }
    return ns;
  };
  const int tseq = tmax > 0 ? tmax : (n_plan >= 100000 ? 128 : 64);
  const int tfus = tmax > 0 ? tmax : (int)std::min<int64_t>(kItemMax, std::max<int64_t>(96, n_plan / 310 / 16 * 16));
  out->n_slots = make_items(tseq, items, multi);
  // the fused launch's items only where its tile shape can apply (hybrid_fused_shape decides per width)
  if (kn.fused_possible && tfus != tseq) out->n_fslots = make_items(tfus, out->fitems, out->fmulti);
  out->n_blocks = (int32_t)bct.size();
  out->dense_nnz = dense;
  const bool same = out->fitems.empty();  // the fused launch walks the same items
  char buf[256];
  snprintf(buf, sizeof(buf), "tiles: %d dense blocks (%dx32, >= %d entries) hold %lld of %lld entries (%.1f %%); %d items, %d split row blocks (fused launch: %d items, %d split)\n",
           out->n_blocks, kTR, th, (long long)dense, (long long)nnz, nnz ? 100.0 * dense / nnz : 0.0, (int)items.size(),
           (int)multi.size(), (int)(same ? items : out->fitems).size(), (int)(same ? multi : out->fmulti).size());
  out->text = buf;
  return WG_OK;
}

}  // namespace wg
