// ids16_check.cpp -- plan_team_ids16 (efficient-gnn_amd/csrc/plan_host.cpp): the 16-bit ids of the team
// waves' leading all-low turns, decoded the way team_dev.h team_wave_spec reads them and compared slot for
// slot with the 32-bit SELL ids, and every wave's n16 against a brute-force count.  Stand-alone: built with
// plan_host.cpp by g++ -fsanitize=address,undefined and run as an ordinary program (tests/test_ids16_plan.py);
// prints "ok ..." and exits 0, or names the first failed check.
#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "plan_host.h"

namespace wg {
int fail(int code, const char*, ...) { return code; }
}  // namespace wg

using namespace wg;
typedef std::vector<int32_t> ivec;

static long g_checks = 0;
static std::string g_ctx;
#define CHECK(cond)                                                                     \
  do {                                                                                  \
    ++g_checks;                                                                         \
    if (!(cond)) {                                                                      \
      std::printf("FAILED %s:%d: %s  [%s]\n", __FILE__, __LINE__, #cond, g_ctx.c_str()); \
      std::exit(1);                                                                     \
    }                                                                                   \
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

// rows given as (low ids, high ids): sorted columns, the low ones in [0, low_lim), the high ones from 65535;
// the rows are put in descending length, as the handle numbers them
struct Rows {
  ivec rs, re, col;
  void finish(std::vector<ivec>& rows) {
    std::stable_sort(rows.begin(), rows.end(), [](const ivec& a, const ivec& b) { return a.size() > b.size(); });
    rs.assign(1, 0);
    for (const ivec& r : rows) {
      col.insert(col.end(), r.begin(), r.end());
      rs.push_back((int32_t)col.size());
    }
    re.assign(rs.begin() + 1, rs.end());
  }
};
static ivec make_row(int n_low, int n_high, int32_t low_lim) {
  ivec r;
  for (int i = 0; i < n_low; ++i) r.push_back((int32_t)(rnd() % (uint32_t)low_lim));
  for (int i = 0; i < n_high; ++i) r.push_back(65535 + (int32_t)(rnd() % 100000u));
  std::sort(r.begin(), r.end());
  return r;
}

static const int32_t* ids_of(const int4& c) { return &c.x; }
static bool low_id(int32_t id) { return id == kPadCol || (id >= 0 && id <= 65534); }

struct Seen {
  long waves = 0, odd = 0, even = 0, all16 = 0, none16 = 0, mixed = 0, parts = 0;
  long first_high_slot[8] = {0, 0, 0, 0, 0, 0, 0, 0};
};

// plans the waves and their 16-bit ids and checks them; returns the totals
static TeamIds16 check(const Rows& g, int LF, int iter, int order, Seen* seen) {
  TeamWaves w;
  CHECK(plan_team_waves(g.rs, g.re, g.col, LF, iter, order, &w) == WG_OK);
  const TeamWaves before = w;
  TeamIds16 h;
  CHECK(plan_team_ids16(&w, LF, &h) == WG_OK);
  const size_t G = (size_t)(64 / LF);
  CHECK(w.sell.size() == before.sell.size() && w.wd.size() == before.wd.size());
  for (size_t i = 0; i < w.sell.size(); ++i)
    for (int j = 0; j < 4; ++j) CHECK(ids_of(w.sell[i])[j] == ids_of(before.sell[i])[j]);  // sell as it was
  std::vector<char> used(h.ids.size(), 0);
  int64_t turns = 0, turns16 = 0;
  for (size_t i = 0; i < w.wd.size(); i += 2) {
    const int4 d0 = w.wd[i], b0 = before.wd[i];
    ctx("LF %d iter %d order %d wave %zu {%d, %d, %d, %#x}", LF, iter, order, i / 2, d0.x, d0.y, d0.z, d0.w);
    CHECK(d0.x == b0.x && d0.y == b0.y && d0.z == b0.z && (d0.w & 0x1ffff) == b0.w && (b0.w >> kIds16Shift) == 0);
    for (int j = 0; j < 4; ++j) CHECK(ids_of(w.wd[i + 1])[j] == ids_of(before.wd[i + 1])[j]);
    const int n16 = (int)((uint32_t)d0.w >> kIds16Shift);
    const size_t x = (size_t)d0.x, ny = (size_t)d0.y;
    // brute force: the leading full turns whose real ids, over all sub-groups, are <= 65534
    int want = 0, first_high = -1;
    for (size_t t = 0; t < ny / 2 && first_high < 0; ++t) {
      for (size_t sg = 0; sg < G && first_high < 0; ++sg)
        for (int s = 0; s < 8 && first_high < 0; ++s)
          if (!low_id(ids_of(w.sell[x + (2 * t + (size_t)(s >> 2)) * G + sg])[s & 3])) first_high = s;
      if (first_high < 0) ++want;
    }
    CHECK(n16 == want);
    CHECK(2 * (size_t)n16 <= ny);
    turns += (int64_t)(ny / 2);
    turns16 += n16;
    ++seen->waves;
    ++(ny & 1 ? seen->odd : seen->even);
    if ((d0.w >> 16) & 1) ++seen->parts;
    if (ny >= 2) ++(n16 == (int)(ny / 2) ? seen->all16 : n16 == 0 ? seen->none16 : seen->mixed);
    if (first_high >= 0) ++seen->first_high_slot[first_high];
    // the converted turns, decoded as the kernel decodes them
    const size_t b = ids16_base((uint32_t)x);
    for (size_t t = 0; t < (size_t)n16; ++t)
      for (size_t sg = 0; sg < G; ++sg) {
        const size_t at = b + t * G + sg;
        CHECK(at < h.ids.size());
        CHECK(!used[at]);  // no two waves share a chunk
        used[at] = 1;
        const uint32_t q[4] = {(uint32_t)h.ids[at].x, (uint32_t)h.ids[at].y, (uint32_t)h.ids[at].z, (uint32_t)h.ids[at].w};
        const uint32_t cc[8] = {q[0] & 0xffffu, q[0] >> 16, q[1] & 0xffffu, q[1] >> 16,
                                q[2] & 0xffffu, q[2] >> 16, q[3] & 0xffffu, q[3] >> 16};
        for (int s = 0; s < 8; ++s) {
          const int32_t id = ids_of(w.sell[x + (2 * t + (size_t)(s >> 2)) * G + sg])[s & 3];
          if (id == kPadCol) CHECK(cc[s] == kIds16Pad);
          else CHECK(cc[s] == (uint32_t)id && cc[s] != kIds16Pad);  // the pad value never stands for a column
        }
      }
  }
  for (size_t i = 0; i < h.ids.size(); ++i)
    if (!used[i]) CHECK(h.ids[i].x == -1 && h.ids[i].y == -1 && h.ids[i].z == -1 && h.ids[i].w == -1);
  CHECK(h.turns == turns && h.turns16 == turns16);
  CHECK(h.ids.empty() == (turns16 == 0));
  if (!h.ids.empty()) CHECK(h.ids.size() == (w.sell.size() + 1) / 2);
  // a second run on the planned table is refused (the counts are in place)
  TeamIds16 again;
  CHECK(turns16 == 0 || plan_team_ids16(&w, LF, &again) != WG_OK);
  return h;
}

int main() {
  const int kLF[3] = {1, 10, 16};
  Seen seen;
  // random graphs: rows of 0 .. 40 low and 0 .. 12 high ids, a few long rows (part waves at iter 32)
  for (int rep = 0; rep < 6; ++rep) {
    std::vector<ivec> rows;
    for (int r = 0; r < 400; ++r) rows.push_back(make_row((int)(rnd() % 41u), rnd() % 3u ? 0 : (int)(rnd() % 13u), 65535));
    for (int r = 0; r < 4; ++r) rows.push_back(make_row(300 + (int)(rnd() % 1500u), (int)(rnd() % 40u), 65535));
    Rows g;
    g.finish(rows);
    for (int LF : kLF)
      for (int iter : {32, 96})
        for (int order : {0, 2}) check(g, LF, iter, order, &seen);
  }
  CHECK(seen.parts > 0 && seen.odd > 0 && seen.even > 0 && seen.all16 > 0 && seen.none16 > 0 && seen.mixed > 0);
  for (int LF : kLF) {
    {  // every id low
      std::vector<ivec> rows;
      for (int r = 0; r < 300; ++r) rows.push_back(make_row(1 + (int)(rnd() % 700u), 0, 3000));
      Rows g;
      g.finish(rows);
      Seen s;
      const TeamIds16 h = check(g, LF, 96, 2, &s);
      CHECK(h.turns16 == h.turns && h.turns > 0 && s.none16 == 0 && s.mixed == 0);
    }
    {  // every id high: no converted turn, no array
      std::vector<ivec> rows;
      for (int r = 0; r < 300; ++r) rows.push_back(make_row(0, 1 + (int)(rnd() % 700u), 3000));
      Rows g;
      g.finish(rows);
      Seen s;
      const TeamIds16 h = check(g, LF, 96, 2, &s);
      CHECK(h.turns16 == 0 && h.turns > 0 && h.ids.empty() && s.all16 == 0 && s.mixed == 0);
    }
    {  // the first high id in each of the eight slots of a turn: a row of 8 t + s low ids and then high ones
      Seen s;
      for (int t = 0; t < 3; ++t)
        for (int q = 0; q < 8; ++q) {
          std::vector<ivec> rows(1, make_row(8 * t + q, 25 - 8 * t - q, 65535));
          Rows g;
          g.finish(rows);
          const TeamIds16 h = check(g, LF, 4096, 0, &s);  // one sub-group on the row: 7 chunks, 3 full turns
          ctx("LF %d first high id at turn %d slot %d", LF, t, q);
          CHECK(h.turns == 3 && h.turns16 == t && s.first_high_slot[q] == t + 1);
        }
    }
    for (int32_t edge : {65534, 65535}) {  // one row of 8 ids ending in the edge column, alone in its wave
      std::vector<ivec> rows(1);
      for (int i = 0; i < 7; ++i) rows[0].push_back(100 + i);
      rows[0].push_back(edge);
      Rows g;
      g.finish(rows);
      Seen s;
      const TeamIds16 h = check(g, LF, 4096, 0, &s);
      ctx("LF %d edge column %d", LF, edge);
      CHECK(h.turns == 1 && h.turns16 == (edge == 65534 ? 1 : 0));
    }
    for (int len : {1, 4, 5, 8, 9, 12, 16, 17}) {  // ny odd and even, a single row
      std::vector<ivec> rows(1, make_row(len, 0, 65535));
      Rows g;
      g.finish(rows);
      Seen s;
      const TeamIds16 h = check(g, LF, 4096, 0, &s);
      ctx("LF %d row of %d", LF, len);
      CHECK(h.turns == (len + 3) / 4 / 2 && h.turns16 == h.turns);
    }
  }
  {  // no rows at all, and a bad width
    Rows g;
    std::vector<ivec> rows;
    g.finish(rows);
    Seen s;
    const TeamIds16 h = check(g, 10, 96, 2, &s);
    CHECK(h.turns == 0 && h.ids.empty());
    TeamWaves w;
    TeamIds16 o;
    CHECK(plan_team_ids16(&w, 0, &o) != WG_OK && plan_team_ids16(&w, 65, &o) != WG_OK);
  }
  std::printf("ok %ld checks, %ld waves (%ld part, %ld odd, %ld even; turns all / none / some converted %ld / %ld / %ld)\n",
              g_checks, seen.waves, seen.parts, seen.odd, seen.even, seen.all16, seen.none16, seen.mixed);
  return 0;
}
