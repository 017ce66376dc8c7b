// plan_check.cpp -- the host planners (efficient-gnn_amd/csrc/plan_host.cpp) on small graphs that hold
// every branch, each table decoded the way its kernel decodes it.  Stand-alone: built together with
// plan_host.cpp by g++ -fsanitize=address,undefined and run as an ordinary program (tests/test_sanitizers.py);
// prints "ok ..." and exits 0, or names the first failed check.
//
// Not covered: plan_team_waves' WG_ERR_UNSUPPORTED at 2^27 id chunks.  The planner tests the limit after it
// has grown the id array, so the case needs a 2 GB allocation however short col is.
#include <algorithm>
#include <array>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "plan_host.h"

namespace wg {
static int g_fail_code = 0;
int fail(int code, const char*, ...) {
  g_fail_code = code;
  return code;
}
}  // namespace wg

using namespace wg;
typedef std::vector<int32_t> ivec;

static long g_checks = 0;
static std::string g_ctx;
#define CHECK(cond)                                                                           \
  do {                                                                                        \
    ++g_checks;                                                                               \
    if (!(cond)) {                                                                            \
      std::printf("FAILED %s:%d: %s  [%s]\n", __FILE__, __LINE__, #cond, g_ctx.c_str());       \
      std::exit(1);                                                                           \
    }                                                                                         \
  } while (0)

static void ctx(const char* fmt, ...) {
  char buf[256];
  va_list ap;
  va_start(ap, fmt);
  std::vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_ctx = buf;
}

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {  // xorshift64*
  g_rng ^= g_rng >> 12;
  g_rng ^= g_rng << 25;
  g_rng ^= g_rng >> 27;
  return (uint32_t)((g_rng * 0x2545F4914F6CDD1Dull) >> 32);
}
static int32_t rnd_below(int64_t n) { return (int32_t)(rnd() % (uint64_t)n); }

struct Graph {
  int64_t n = 0, n_cols = 0;
  ivec rp, col;
  int64_t len(int64_t r) const { return rp[r + 1] - rp[r]; }
};

// Rows in descending length: one hub row of hub_len entries, lengths falling to 14, every length from 13 to
// 0 (both sides of each multiple of 4 up to 12), a block of empty rows at the end.  Columns in [0, col_lim);
// distinct: no column twice in a row (lengths capped at col_lim), in random order.
static Graph make_graph(int64_t n, int64_t n_cols, int64_t col_lim, int64_t hub_len, int64_t max_len, bool distinct) {
  Graph g;
  g.n = n;
  g.n_cols = n_cols;
  ivec len(n, 0);
  const int64_t nz = n < 40 ? n : n - n / 10;
  for (int64_t r = 0; r < nz; ++r) {
    if (r == 0) len[r] = (int32_t)hub_len;
    else if (n < 40) len[r] = (int32_t)std::max<int64_t>(0, 13 - 5 * (r - 1));  // 13, 8, 3, 0
    else if (r >= nz - 28) len[r] = (int32_t)((nz - 1 - r) / 2);                // 13, 13, 12, 12, ... 0, 0
    else {
      const int64_t m = nz - 28, d = m - r;
      len[r] = (int32_t)(14 + (max_len - 14) * d * d / (m * m));
    }
    if (col_lim == 0) len[r] = 0;
    else if (distinct) len[r] = (int32_t)std::min<int64_t>(len[r], col_lim);
  }
  std::sort(len.begin(), len.end(), [](int32_t a, int32_t b) { return a > b; });
  g.rp.assign(n + 1, 0);
  for (int64_t r = 0; r < n; ++r) g.rp[r + 1] = g.rp[r] + len[r];
  g.col.resize(g.rp[n]);
  ivec pool(distinct ? col_lim : 0);
  for (size_t i = 0; i < pool.size(); ++i) pool[i] = (int32_t)i;
  for (int64_t r = 0; r < n; ++r)
    for (int32_t i = 0; i < len[r]; ++i) {
      if (distinct) {  // a partial Fisher-Yates shuffle: the first len[r] of pool
        std::swap(pool[i], pool[i + rnd_below(col_lim - i)]);
        g.col[g.rp[r] + i] = pool[i];
      } else {
        // clustered low columns on the long rows, so that dense tiles exist
        g.col[g.rp[r] + i] = rnd_below(rnd() & 1 ? col_lim : std::max<int64_t>(1, col_lim / 8));
      }
    }
  return g;
}

static bool is_pad4(const int4& c) { return c.x == kPadCol && c.y == kPadCol && c.z == kPadCol && c.w == kPadCol; }

// one decoded id: its place in the row (part, chunk, lane of the chunk) and the id
struct Slot {
  int64_t part, chunk;
  int j;
  int32_t id;
  bool operator<(const Slot& o) const {
    return part != o.part ? part < o.part : chunk != o.chunk ? chunk < o.chunk : j < o.j;
  }
};
static void push_chunk(std::vector<Slot>& v, int64_t part, int64_t chunk, const int4& c) {
  const int32_t id[4] = {c.x, c.y, c.z, c.w};
  for (int j = 0; j < 4; ++j) v.push_back(Slot{part, chunk, j, id[j]});
}
// the decoded slots of a row, put in place: the row's entries in order, then pads only
static void check_row(std::vector<Slot>& v, const ivec& col, int64_t e0, int64_t e1) {
  std::sort(v.begin(), v.end());
  CHECK((int64_t)v.size() >= e1 - e0);
  for (size_t i = 0; i < v.size(); ++i) CHECK(v[i].id == ((int64_t)i < e1 - e0 ? col[e0 + (int64_t)i] : kPadCol));
}

// ---------------------------------------------------------------------------------------------------------
// plan_team_waves (decoded as team_dev.h team_wave + step_dev.h accumulate_sell) and plan_team_first
// ---------------------------------------------------------------------------------------------------------
typedef std::vector<std::array<int32_t, 8>> WaveKeys;
static WaveKeys wave_keys(const TeamWaves& t) {
  WaveKeys k;
  for (size_t w = 0; w + 1 < t.wd.size(); w += 2)
    k.push_back({t.wd[w].x, t.wd[w].y, t.wd[w].z, t.wd[w].w, t.wd[w + 1].x, t.wd[w + 1].y, t.wd[w + 1].z, t.wd[w + 1].w});
  std::sort(k.begin(), k.end());
  return k;
}

static void check_team(const ivec& rs, const ivec& re, const ivec& col, int LF, int iter, TeamWaves* keep = nullptr) {
  const int64_t n = (int64_t)re.size();
  const int G = 64 / LF;
  const int64_t tch = std::max<int64_t>(2, (iter / 4 + 1) / 2 * 2);  // chunks per sub-group a wave aims at
  TeamWaves t;
  CHECK(plan_team_waves(rs, re, col, LF, iter, 0, &t) == WG_OK);
  CHECK(t.wd.size() % 2 == 0);
  const int64_t nw = (int64_t)t.wd.size() / 2;
  CHECK(t.sell.size() >= (size_t)4 * G);
  const int64_t body = (int64_t)t.sell.size() - 4 * G;
  for (int64_t i = body; i < (int64_t)t.sell.size(); ++i) CHECK(is_pad4(t.sell[i]));  // the read-ahead tail
  std::vector<std::vector<Slot>> rows(n);
  std::vector<int> covered(n, 0);
  struct Long { int32_t parts, slot, counter, seen; };
  std::map<int64_t, Long> longs;
  int64_t next = 0, real_ids = 0;
  for (int64_t w = 0; w < nw; ++w) {
    const int4 d0 = t.wd[2 * w], d1 = t.wd[2 * w + 1];
    const int LN = d0.w & 0xff, tpw = (d0.w >> 8) & 0xff, part = (d0.w >> 16) & 1;
    CHECK((d0.w >> 17) == 0);
    CHECK(LN >= 1 && G % LN == 0 && tpw >= 1 && tpw * LN <= G);
    CHECK(d0.x == next && d0.y >= 0 && (int64_t)d0.x + (int64_t)d0.y * G <= body);  // waves tile sell in order
    next += (int64_t)d0.y * G;
    CHECK(d0.z >= 0 && (int64_t)d0.z + tpw <= n);
    if (part) {
      CHECK(LN == G && tpw == 1);
      CHECK(d1.y >= 2 && d1.x >= 0 && d1.x < d1.y);
      auto it = longs.find(d0.z);
      if (it == longs.end()) it = longs.insert({d0.z, Long{d1.y, d1.z, d1.w, 0}}).first;
      Long& L = it->second;
      CHECK(L.parts == d1.y && L.slot == d1.z && L.counter == d1.w);  // one first slot, one counter
      CHECK(d1.x == L.seen);                                          // parts 0 .. parts-1, in order
      ++L.seen;
      const int64_t nch = (re[d0.z] - rs[d0.z] + 3) / 4, per = (int64_t)G * tch;
      CHECK(nch > per && d1.y == (nch + per - 1) / per);
      const int64_t share = std::min(nch, (d1.x + 1) * per) - d1.x * per;
      CHECK((int64_t)d0.y * G >= share);  // every sub-group's chunks fit
    } else {
      CHECK(d1.x == 0 && d1.y == 0 && d1.z == 0 && d1.w == 0);
      for (int i = 0; i < tpw; ++i) {
        ++covered[d0.z + i];
        const int64_t nch = (re[d0.z + i] - rs[d0.z + i] + 3) / 4;
        CHECK((int64_t)d0.y * LN >= nch);  // sub-group 0 holds the most: ceil(nch / LN)
      }
    }
    for (int sg = 0; sg < G; ++sg) {
      const int team = sg / LN, ns = sg - team * LN;
      for (int64_t k = 0; k < d0.y; ++k) {
        const int4 c = t.sell[(size_t)d0.x + (size_t)k * G + sg];
        if (team >= tpw) CHECK(is_pad4(c));  // an idle sub-group
        else if (part) push_chunk(rows[d0.z], d1.x, k * G + sg, c);
        else push_chunk(rows[d0.z + team], 0, ns + k * LN, c);
        real_ids += (c.x != kPadCol) + (c.y != kPadCol) + (c.z != kPadCol) + (c.w != kPadCol);
      }
    }
  }
  CHECK(next == body);
  int64_t nnz = 0;
  int32_t slots = 0, counters = 0, max_parts = 0, npot = 0;
  for (int64_t r = 0; r < n; ++r) {
    auto it = longs.find(r);
    if (it != longs.end()) {
      const Long& L = it->second;
      CHECK(covered[r] == 0 && L.seen == L.parts);
      CHECK(L.slot == slots && L.counter == counters);  // dense in [0, n_slots) and [0, n_long)
      slots += L.parts;
      ++counters;
      max_parts = std::max(max_parts, L.parts);
      if (L.parts & (L.parts - 1)) ++npot;
    } else {
      CHECK(covered[r] == 1);
    }
    check_row(rows[r], col, rs[r], re[r]);
    nnz += re[r] - rs[r];
  }
  CHECK(real_ids == nnz);
  CHECK(t.n_slots == slots && t.n_long == counters && t.max_parts == max_parts && t.npot_rows == npot);
  const WaveKeys k0 = wave_keys(t);
  for (int order = 1; order <= 7; ++order) {  // the dispatch orders permute the waves, nothing else
    TeamWaves o;
    CHECK(plan_team_waves(rs, re, col, LF, iter, order, &o) == WG_OK);
    CHECK(o.sell.size() == t.sell.size() && std::memcmp(o.sell.data(), t.sell.data(), sizeof(int4) * t.sell.size()) == 0);
    CHECK(wave_keys(o) == k0);
    CHECK(o.n_slots == t.n_slots && o.n_long == t.n_long && o.max_parts == t.max_parts && o.npot_rows == t.npot_rows);
    if (order == 1 && nw > 0) CHECK(o.wd[0].x == t.wd[2 * (nw - 1)].x && o.wd[0].z == t.wd[2 * (nw - 1)].z);
  }
  if (keep) *keep = std::move(t);
}

static void check_team_first(const TeamWaves& t, int64_t n_rows, int64_t n_cols) {
  ivec perm(n_rows);
  for (int64_t i = 0; i < n_rows; ++i) perm[i] = (int32_t)i;
  for (int64_t i = n_rows - 1; i > 0; --i) std::swap(perm[i], perm[rnd_below(i + 1)]);
  std::vector<double> dinv(n_cols);
  for (auto& d : dinv) d = 1.0 / (1.0 + rnd_below(1000));
  TeamFirstIds f;
  CHECK(plan_team_first(t.sell, perm, dinv, &f) == WG_OK);
  CHECK(f.sell0.size() == t.sell.size() && f.sdinv.size() == 4 * t.sell.size());
  for (size_t i = 0; i < t.sell.size(); ++i) {
    const int32_t a[4] = {t.sell[i].x, t.sell[i].y, t.sell[i].z, t.sell[i].w};
    const int32_t b[4] = {f.sell0[i].x, f.sell0[i].y, f.sell0[i].z, f.sell0[i].w};
    for (int j = 0; j < 4; ++j) {
      if (a[j] == kPadCol) CHECK(b[j] == kPadCol && f.sdinv[4 * i + j] == 0.0);
      else CHECK(b[j] == perm[a[j]] && f.sdinv[4 * i + j] == dinv[a[j]]);
    }
  }
  std::vector<int4> bad = t.sell;  // an id past the rows (a halo column): not a caller row
  bad[0].y = (int32_t)n_rows;
  g_fail_code = 0;
  CHECK(plan_team_first(bad, perm, dinv, &f) == WG_ERR_INVALID && g_fail_code == WG_ERR_INVALID);
  bad[0].y = -1;
  CHECK(plan_team_first(bad, perm, dinv, &f) == WG_ERR_INVALID);
}

// ---------------------------------------------------------------------------------------------------------
// plan_segments + plan_sell (decoded as step_dev.h cheb_step_kernel's units) and plan_pcol
// ---------------------------------------------------------------------------------------------------------
static void fill_buckets(const Graph& g, unsigned int* bucket) {
  for (int b = 0; b < kBuckets; ++b) bucket[b] = 0;
  for (int64_t r = 0; r < g.n; ++r) {
    int b = 0;
    while (b < 32 && (int64_t)1 << b < g.len(r)) ++b;  // ceil(log2 len), 0 for len <= 1
    ++bucket[b];
  }
}

static void check_seg_table(const SegKnobs& kn, int64_t n, const SegPlan& sp) {
  const SegTable& t = sp.tab;
  CHECK(t.n >= 0 && t.n <= kMaxSeg);
  int32_t blk = 0;
  int64_t row = sp.n_split;
  for (int i = 0; i < t.n; ++i) {
    const Seg& s = t.s[i];
    CHECK(s.blk_begin == blk);  // non-decreasing, each segment after the one before
    CHECK(s.ln >= 1 && kn.G % s.ln == 0 && s.end >= s.begin);
    if (s.mode == 2) {
      CHECK(i == 0 && s.begin == 0 && s.end == (int32_t)sp.chunks.size() && sp.n_split > 0);
      blk += s.end;
    } else {
      CHECK(s.mode == 0 || s.mode == 1);
      CHECK(s.begin == row);  // the rows after the split rows, in order
      row = s.end;
      blk += s.mode == 1 ? s.end - s.begin : (int32_t)ceil_div(s.end - s.begin, (int64_t)kn.NW * (kn.G / s.ln));
      if (s.mode == 1) CHECK(i == (sp.n_split > 0 ? 1 : 0));
    }
  }
  CHECK(t.total_blocks == blk);
  CHECK(row == n);
  if (n > 0) CHECK(!sp.text.empty());
}

static void check_segments(const Graph& g, int LF, int NW, int iter, int block_iter, int chunk_iter) {
  SegKnobs kn;
  kn.G = 64 / LF;
  kn.NW = NW;
  kn.iter = iter;
  kn.block_iter = block_iter;
  kn.chunk_iter = chunk_iter;
  unsigned int bucket[kBuckets];
  fill_buckets(g, bucket);
  const int64_t n = g.n, G = kn.G, n_split = count_split_rows(kn, bucket);
  SegPlan sp;
  if (n_split > 0) {  // the row starts are needed, and asked for
    g_fail_code = 0;
    CHECK(plan_segments(kn, n, bucket, ivec(), &sp) == WG_ERR_INVALID && g_fail_code == WG_ERR_INVALID);
  }
  CHECK(plan_segments(kn, n, bucket, ivec(g.rp.begin(), g.rp.begin() + (n_split ? n_split + 1 : 0)), &sp) == WG_OK);
  CHECK(sp.n_split == n_split);
  check_seg_table(kn, n, sp);
  // split chunks partition each split row's entries in order; rowchunks index them
  const int64_t CH = (int64_t)NW * G * chunk_iter;
  CHECK((int64_t)sp.rowchunks.size() == n_split);
  int32_t c = 0;
  for (int64_t r = 0; r < n_split; ++r) {
    CHECK(sp.rowchunks[r].x == c && sp.rowchunks[r].y >= 1);
    CHECK(g.len(r) > (int64_t)NW * G * block_iter / 2);  // a split row is one of a long bucket
    int32_t e = g.rp[r];
    for (int q = 0; q < sp.rowchunks[r].y; ++q, ++c) {
      CHECK(c < (int32_t)sp.chunks.size());
      const ChunkDesc& d = sp.chunks[c];
      CHECK(d.row == r && d.e0 == e && d.e1 > d.e0 && d.e1 - d.e0 <= CH && d.pad == 0);
      e = d.e1;
    }
    CHECK(e == g.rp[r + 1]);
  }
  CHECK(c == (int32_t)sp.chunks.size());
  // the team segments' SELL table
  SellTable st;
  CHECK(plan_sell(sp.tab, NW, LF, g.rp, g.col, &st) == WG_OK);
  CHECK((int64_t)st.wmeta.size() == (int64_t)sp.tab.total_blocks * NW);
  CHECK(st.sell.size() >= (size_t)4 * G);
  const int64_t body = (int64_t)st.sell.size() - 4 * G;
  for (int64_t i = body; i < (int64_t)st.sell.size(); ++i) CHECK(is_pad4(st.sell[i]));
  int64_t next = 0, real_ids = 0, team_nnz = 0;
  std::vector<Slot> slots;
  for (int si = 0; si < sp.tab.n; ++si) {
    const Seg& s = sp.tab.s[si];
    const int32_t nblk = (si + 1 < sp.tab.n ? sp.tab.s[si + 1].blk_begin : sp.tab.total_blocks) - s.blk_begin;
    if (s.mode != 0) {
      for (int64_t w = (int64_t)s.blk_begin * NW; w < (int64_t)(s.blk_begin + nblk) * NW; ++w)
        CHECK(st.wmeta[w].x == 0 && st.wmeta[w].y == 0);
      continue;
    }
    const int LN = s.ln, tpw = (int)G / LN;
    for (int32_t u = 0; u < nblk; ++u)
      for (int w = 0; w < NW; ++w) {
        const int2 m = st.wmeta[(size_t)(s.blk_begin + u) * NW + w];
        CHECK(m.x == next && m.y >= 0 && m.y % 2 == 0 && (int64_t)m.x + (int64_t)m.y * G <= body);
        next += (int64_t)m.y * G;
        const int64_t r0 = (int64_t)s.begin + ((int64_t)u * NW + w) * tpw;
        for (int t = 0; t < (int)G / LN; ++t) {
          const int64_t r = r0 + t;
          slots.clear();
          for (int ns = 0; ns < LN; ++ns) {
            const int sg = t * LN + ns;
            for (int64_t k = 0; k < m.y; ++k) {
              const int4 ch = st.sell[(size_t)m.x + (size_t)k * G + sg];
              if (r >= s.end) CHECK(is_pad4(ch));  // past the segment: an idle sub-group
              else push_chunk(slots, 0, ns + k * LN, ch);
              real_ids += (ch.x != kPadCol) + (ch.y != kPadCol) + (ch.z != kPadCol) + (ch.w != kPadCol);
            }
          }
          if (r >= s.end) continue;
          CHECK((int64_t)m.y * LN >= (g.len(r) + 3) / 4);  // covers the longest sub-group
          check_row(slots, g.col, g.rp[r], g.rp[r + 1]);
          team_nnz += g.len(r);
        }
      }
  }
  CHECK(next == body && real_ids == team_nnz);
}

// more bucket-sized team segments than the table holds: the last one is extended.  Reached only with a wide
// divisor set, so G = 2^24 here (bucket counts alone: no rows are read without split rows)
static void check_segments_overflow() {
  ctx("segments overflow");
  SegKnobs kn;
  kn.G = 1 << 24;
  kn.NW = 4;
  kn.iter = 1;
  kn.block_iter = 1 << 20;
  kn.chunk_iter = 1;
  unsigned int bucket[kBuckets] = {0};
  int64_t n = 0;
  for (int b = 0; b <= 24; ++b) n += bucket[b] = 3 + b;  // 25 different team sizes: 1, 2, 4, ... 2^24
  CHECK(count_split_rows(kn, bucket) == 0);
  SegPlan sp;
  CHECK(plan_segments(kn, n, bucket, ivec(), &sp) == WG_OK);
  CHECK(sp.tab.n == kMaxSeg);
  check_seg_table(kn, n, sp);
  kn.reordered = false;  // caller order: one segment
  kn.avg_len = 3;
  CHECK(plan_segments(kn, n, bucket, ivec(), &sp) == WG_OK);
  CHECK(sp.tab.n == 1 && sp.tab.s[0].begin == 0 && sp.tab.s[0].end == n && sp.tab.s[0].ln == 4);
  check_seg_table(kn, n, sp);
}

static void check_pcol(const Graph& g) {
  PaddedCsr p;
  CHECK(plan_pcol(g.rp, g.col, &p) == WG_OK);
  CHECK((int64_t)p.prp.size() == g.n + 1 && p.prp[0] == 0);
  for (int64_t r = 0; r < g.n; ++r) {
    CHECK(p.prp[r + 1] >= p.prp[r] && (p.prp[r + 1] - p.prp[r]) % 4 == 0);
    CHECK(p.prp[r + 1] - p.prp[r] == (g.len(r) + 3) / 4 * 4);
    for (int32_t i = 0; i < p.prp[r + 1] - p.prp[r]; ++i)
      CHECK(p.pcol[p.prp[r] + i] == (i < g.len(r) ? g.col[g.rp[r] + i] : kPadCol));
  }
  CHECK((int64_t)p.pcol.size() == (int64_t)p.prp[g.n] + kPcolTail);
  for (size_t i = p.prp[g.n]; i < p.pcol.size(); ++i) CHECK(p.pcol[i] == kPadCol);
}

// ---------------------------------------------------------------------------------------------------------
// plan_tiles (decoded as tiles.hip cheb_tiles_kernel's items and the step kernel's phase-4 tail)
// ---------------------------------------------------------------------------------------------------------
// items (and multi) cover every row block's blocks once and in order; fills each block's row block
static void check_items(const std::vector<int4>& items, const std::vector<int4>& multi, int32_t n_blocks, int32_t n_slots,
                        int tm, int64_t n_rb, ivec* block_rb) {
  int32_t b = 0, ns = 0;
  size_t m = 0, i = 0;
  int32_t last_rb = -1;
  block_rb->assign(n_blocks, -1);
  while (i < items.size()) {
    const int32_t rb = items[i].x;
    CHECK(rb > last_rb && rb < n_rb);
    last_rb = rb;
    size_t j = i;
    while (j < items.size() && items[j].x == rb) ++j;
    const int32_t k = (int32_t)(j - i);
    for (size_t q = i; q < j; ++q) {
      CHECK(items[q].y == b && items[q].z > b && items[q].z - b <= tm && items[q].z <= n_blocks);
      CHECK(items[q].w == (k == 1 ? -1 : ns + (int32_t)(q - i)));
      for (; b < items[q].z; ++b) (*block_rb)[b] = rb;
    }
    if (k > 1) {
      CHECK(m < multi.size() && multi[m].x == rb && multi[m].y == ns && multi[m].z == k && multi[m].w == 0);
      ++m;
      ns += k;
    }
    i = j;
  }
  CHECK(b == n_blocks && m == multi.size() && ns == n_slots);
}

static void check_tiles(const Graph& g, int64_t n_plan, int64_t col_limit, const TileKnobs& kn, bool expect_dense) {
  TileTables t;
  CHECK(plan_tiles(g.rp, g.col, n_plan, g.n_cols, col_limit, kn, &t) == WG_OK);
  const int TR = kn.rows;
  const int64_t n_rb = ceil_div(n_plan, TR);
  CHECK(t.n_blocks == (int32_t)t.bct.size() && t.bmask.size() == t.bct.size() * (size_t)TR);
  CHECK((int64_t)t.tsplit.size() == g.n && t.tcol.size() == g.col.size());
  if (expect_dense) CHECK(t.n_blocks > 0);
  const int tseq = kn.tile_max > 0 ? kn.tile_max : 64;  // n_plan < 100 000 rows
  const int tfus = kn.tile_max > 0 ? kn.tile_max : 96;  // n_plan / 310 < 96
  ivec block_rb, fblock_rb;
  check_items(t.items, t.multi, t.n_blocks, t.n_slots, std::min(tseq, kItemMax), n_rb, &block_rb);
  if (!kn.fused_possible || tfus == tseq) {
    CHECK(t.fitems.empty() && t.fmulti.empty() && t.n_fslots == 0);
  } else {
    check_items(t.fitems, t.fmulti, t.n_blocks, t.n_fslots, tfus, n_rb, &fblock_rb);
    CHECK(fblock_rb == block_rb);
  }
  std::vector<std::vector<int32_t>> rb_blocks(n_rb);
  int64_t dense = 0;
  for (int32_t b = 0; b < t.n_blocks; ++b) {
    const int32_t rb = block_rb[b];
    if (!rb_blocks[rb].empty()) CHECK(t.bct[b] > t.bct[rb_blocks[rb].back()]);  // ascending within a row block
    rb_blocks[rb].push_back(b);
    CHECK(t.bct[b] >= 0 && (int64_t)t.bct[b] * kTC < col_limit);
    int64_t in_block = 0;
    for (int rl = 0; rl < TR; ++rl) {
      const uint32_t m = t.bmask[(size_t)b * TR + rl];
      if ((int64_t)rb * TR + rl >= n_plan) CHECK(m == 0);  // the partial last row block
      in_block += __builtin_popcount(m);
    }
    CHECK(in_block >= kn.th);
    dense += in_block;
  }
  CHECK(dense == t.dense_nnz);
  ivec got, want, tail_cnt(ceil_div(g.n_cols, kTC), 0);  // tail entries per column tile of the row block
  for (int64_t r = 0; r < g.n; ++r) {
    CHECK(t.tsplit[r] >= g.rp[r] && t.tsplit[r] <= g.rp[r + 1]);
    if (r < n_plan) {  // what stays in the tail made no dense block: fewer than th entries per tile
      if (r % TR == 0) std::fill(tail_cnt.begin(), tail_cnt.end(), 0);
      for (int32_t e = g.rp[r]; e < t.tsplit[r]; ++e) CHECK(++tail_cnt[t.tcol[e] / kTC] < kn.th);
    }
    if (r >= n_plan) {  // unplanned: all tail, the operator's own order
      CHECK(t.tsplit[r] == g.rp[r + 1]);
      for (int32_t e = g.rp[r]; e < g.rp[r + 1]; ++e) CHECK(t.tcol[e] == g.col[e]);
      continue;
    }
    got.assign(t.tcol.begin() + g.rp[r], t.tcol.begin() + t.tsplit[r]);
    for (int32_t b : rb_blocks[r / TR]) {
      const uint32_t m = t.bmask[(size_t)b * TR + (r % TR)];
      for (int k = 0; k < kTC; ++k)
        if (m >> k & 1) got.push_back(t.bct[b] * kTC + k);
    }
    want.assign(g.col.begin() + g.rp[r], g.col.begin() + g.rp[r + 1]);
    std::sort(got.begin(), got.end());
    std::sort(want.begin(), want.end());
    CHECK(got == want);  // tail + mask bits = the row's columns (no column twice in a row)
  }
  CHECK(t.text.compare(0, 6, "tiles:") == 0);
}

static void check_tiles_refusals() {
  ctx("tiles refusals");
  Graph g = make_graph(300, 300, 300, 200, 120, true);
  TileKnobs kn;
  kn.th = 1;
  kn.rows = 64;
  TileTables t;
  Graph dup = g;  // a repeated entry inside a dense block: no plan, no error
  dup.col[dup.rp[3] + 1] = dup.col[dup.rp[3]];
  CHECK(plan_tiles(dup.rp, dup.col, dup.n, dup.n_cols, dup.n_cols, kn, &t) == WG_OK);
  CHECK(t.n_blocks == 0 && t.bct.empty() && t.items.empty());
  Graph out = g;  // a column past the limit
  out.col[out.rp[2]] = 299;
  g_fail_code = 0;
  CHECK(plan_tiles(out.rp, out.col, out.n, out.n_cols, 299, kn, &t) == WG_ERR_INVALID && g_fail_code == WG_ERR_INVALID);
  out.col[out.rp[2]] = -1;
  CHECK(plan_tiles(out.rp, out.col, out.n, out.n_cols, 300, kn, &t) == WG_ERR_INVALID);
  // no dense block at all: one entry per row, spread over the tiles
  Graph sp;
  sp.n = sp.n_cols = 300;
  sp.rp.resize(301);
  sp.col.resize(300);
  for (int r = 0; r < 300; ++r) {
    sp.rp[r + 1] = r + 1;
    sp.col[r] = r * 37 % 300;
  }
  kn.th = 16;
  kn.rows = 128;
  kn.fused_possible = true;
  CHECK(plan_tiles(sp.rp, sp.col, 300, 300, 300, kn, &t) == WG_OK);
  CHECK(t.n_blocks == 0 && t.items.empty() && t.fitems.empty() && t.dense_nnz == 0);
  for (int r = 0; r < 300; ++r) CHECK(t.tsplit[r] == sp.rp[r + 1] && t.tcol[r] == sp.col[r]);
}

int main() {
  const int64_t ns[] = {0, 1, 5, 300, 1000};
  const int lfs[] = {1, 10, 12, 16}, iters[] = {8, 96, 128}, nws[] = {4, 8};
  for (int64_t n : ns)
    for (int halo = 0; halo < 2; ++halo) {
      const int64_t n_cols = n + (halo ? 200 : 0);
      // team waves: a hub of 3 part waves for each (LF, iter); columns may repeat
      for (int LF : lfs)
        for (int iter : iters) {
          const int G = 64 / LF;
          const int64_t tch = std::max<int64_t>(2, (iter / 4 + 1) / 2 * 2);
          const Graph g = make_graph(n, n_cols, n_cols, 4 * (2 * G * tch + 5), 120, false);
          const ivec ends(g.rp.begin() + 1, g.rp.end());
          ctx("team waves n=%lld cols=%lld LF=%d iter=%d", (long long)n, (long long)n_cols, LF, iter);
          TeamWaves t;
          check_team(g.rp, ends, g.col, LF, iter, &t);
          if (n > 0 && n_cols > 0) CHECK(t.n_long >= 1 && t.max_parts >= 3 && t.npot_rows >= 1);  // the hub: 3 parts
          if (!halo && n > 0) check_team_first(t, n, n_cols);
          ivec tails(n);  // the hybrid step's tail ends: anywhere in the row, so not monotone
          for (int64_t r = 0; r < n; ++r) tails[r] = g.rp[r] + rnd_below(g.len(r) + 1);
          ctx("team waves, tail ends n=%lld cols=%lld LF=%d iter=%d", (long long)n, (long long)n_cols, LF, iter);
          check_team(g.rp, tails, g.col, LF, iter);
          for (int NW : nws) {
            // the hub as a block row, then as a split row of several chunks (block rows may not be shorter
            // than team rows, NW * block_iter >= iter: the classification counts such a bucket twice)
            ctx("segments n=%lld cols=%lld LF=%d iter=%d NW=%d", (long long)n, (long long)n_cols, LF, iter, NW);
            check_segments(g, LF, NW, iter, iter, std::max(1, iter / 4));
            const int bi = (iter + NW - 1) / NW;
            check_segments(g, LF, NW, iter, bi, std::max(1, bi / 2));
          }
        }
      const Graph g = make_graph(n, n_cols, n_cols, 1100, 120, false);
      ctx("pcol n=%lld cols=%lld", (long long)n, (long long)n_cols);
      check_pcol(g);
      // tiles: every row planned, and the active rows only (a whole graph's closed rows end the column space)
      for (int active = 0; active < 2; ++active) {
        const int64_t n_plan = active ? n - n / 10 : n;
        const int64_t col_limit = (active && !halo) ? n_plan : n_cols;
        const Graph gt = make_graph(n, n_cols, col_limit, 1100, n >= 1000 ? 250 : 200, true);
        for (int rows : {64, 128})
          for (int th : {1, 16, 96})
            for (int tile_max : {0, 1, 3})
              for (int fused = 0; fused < (rows == 128 ? 2 : 1); ++fused) {  // the fused launch: 128-row blocks only
                TileKnobs kn;
                kn.th = th;
                kn.tile_max = tile_max;
                kn.rows = rows;
                kn.fused_possible = fused;
                ctx("tiles n=%lld cols=%lld plan=%lld rows=%d th=%d max=%d fused=%d", (long long)n, (long long)n_cols,
                    (long long)n_plan, rows, th, tile_max, fused);
                check_tiles(gt, n_plan, col_limit, kn, n >= 300);
              }
      }
    }
  check_segments_overflow();
  check_tiles_refusals();
  std::printf("ok %ld checks\n", g_checks);
  return 0;
}
