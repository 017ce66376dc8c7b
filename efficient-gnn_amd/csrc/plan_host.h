// plan_host.h -- the host-side planners of the step kernels' tables (plan_host.cpp) and the constants
// and table structs the tables share with the kernels.  Host-only: no HIP runtime header, no device
// handle -- each planner maps the host CSR (row starts, row ends where they differ, column ids) and a
// few plain knobs to vectors, so it builds with any C++17 compiler and runs under ASan / UBSan
// (tests/c/plan_check.cpp).  The .hip builders download the CSR, call a planner and upload its result.
#pragma once

#include <hip/hip_vector_types.h>  // int2 / int4 only

#include <cstdint>
#include <string>
#include <vector>

#include "wats_hip.h"

namespace wg {

int fail(int code, const char* fmt, ...);  // the library's definition: capi.hip

constexpr int kMaxSeg = 24;
constexpr int kBuckets = 33;  // row-length buckets: b=0: len<=1; b>0: 2^(b-1) < len <= 2^b
// a padded-CSR column id whose byte offset (id * row bytes <= 256) lies past every gathered buffer
constexpr int32_t kPadCol = 0xFFFFFF;
// kPadCol ids after the last row of pcol: a sub-group's id loads run up to (PF + 1) turns of CPT
// steps (<= 4096 ids each) past its range
constexpr int32_t kPcolTail = 65536;
constexpr int kTC = 32;         // hybrid step: columns per tile (the MFMA's K)
constexpr int kItemMax = 1024;  // hybrid step: dense blocks per work item (tile_max <= 1024)

inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

// ---------------------------------------------------------------------------
// Step-kernel launch plan (per signal-tile shape), see step.hip.
// ---------------------------------------------------------------------------
struct Seg {
  int32_t begin;      // team mode: internal rows [begin, end); chunk mode: chunk ids
  int32_t end;
  int32_t blk_begin;  // first workgroup of this segment
  int32_t ln;         // team mode: lane sub-groups cooperating on one row
  int32_t mode;       // 0 = team, 1 = block (workgroup per row), 2 = split (workgroup per nnz chunk)
};

struct SegTable {
  Seg s[kMaxSeg];
  int32_t n;
  int32_t total_blocks;
};

struct ChunkDesc {  // one workgroup's share of a split row
  int32_t row;
  int32_t e0, e1;   // nnz range
  int32_t pad;
};

// team.hip: the wave table (two int4 per wave) and SELL ids of rows [0, n), n = rs.size() - 1; the
// entries of row r are col[rs[r] .. re[r])
struct TeamWaves {
  std::vector<int4> wd, sell;
  int32_t n_slots = 0, n_long = 0, max_parts = 0, npot_rows = 0;
};
int plan_team_waves(const std::vector<int32_t>& rs, const std::vector<int32_t>& re, const std::vector<int32_t>& col,
                    int LF, int iter, int order, TeamWaves* out);

// team.hip: 16-bit column ids for a wave's leading full turns whose real ids are all <= 65534
// (team_dev.h team_wave_spec).  n16, the count of such turns, goes into bits
// kIds16Shift and up of the wave's d0.w; turn t < n16 of sub-group sg is the one 16-B chunk
// ids[ids16_base(d0.x) + t G + sg], the turn's eight ids in the slot order {c0.x .. c0.w, c1.x .. c1.w}
// (slot s in half s & 1 of word s >> 1), pads kIds16Pad.  sell is left as it is.  The base needs no
// descriptor field: a wave's ny G chunks of sell leave room for its <= ny / 2 turns of G chunks at
// half its own offset, rounded up.  ids stays empty when no wave has such a turn.
constexpr uint32_t kIds16Pad = 0xFFFF;
constexpr int kIds16Shift = 17;
constexpr int kIds16Max = (1 << 14) - 1;  // d0.w bits 17 .. 30
constexpr uint32_t ids16_base(uint32_t first_chunk) { return (first_chunk + 1u) >> 1; }
struct TeamIds16 {
  std::vector<int4> ids;
  int64_t turns16 = 0, turns = 0;  // converted turns; full turns of all waves
};
int plan_team_ids16(TeamWaves* w, int LF, TeamIds16* out);

// team.hip: the folded chain's first-launch ids (caller rows) and each id slot's dinv; sell (the wave
// table's ids) is moved in and mapped in place
struct TeamFirstIds {
  std::vector<int4> sell0;
  std::vector<double> sdinv;
};
int plan_team_first(std::vector<int4> sell, const std::vector<int32_t>& perm, const std::vector<double>& dinv,
                    TeamFirstIds* out);

// step.hip: the segment table of rows [0, n) sorted by descending length (bucket: rows per length
// bucket) and the split rows' chunk tables; rp: row starts of at least the split rows
struct SegKnobs {
  int G = 64, NW = 4;
  int iter = 0, block_iter = 0, chunk_iter = 0;  // default_knobs
  bool reordered = true;
  int64_t avg_len = 0;  // caller order: the one segment is sized by it
};
struct SegPlan {
  SegTable tab{};
  int32_t n_split = 0;  // split rows = rows [0, n_split)
  std::vector<ChunkDesc> chunks;
  std::vector<int2> rowchunks;  // [n_split] {first chunk, chunk count}
  std::string text;
};
void default_knobs(int t_iter, int t_block_iter, int t_chunk_iter, int G, int64_t nnz, int* iter, int* block_iter,
                   int* chunk_iter, bool hybrid = false, int64_t rows = 0);
int divisor_at_least(int G, int64_t want);
int64_t count_split_rows(const SegKnobs& k, const unsigned int* bucket);  // rp must hold their row starts
int plan_segments(const SegKnobs& k, int64_t n, const unsigned int* bucket, const std::vector<int32_t>& rp,
                  SegPlan* out);

// step.hip: the SELL order of a segment table's team waves
struct SellTable {
  std::vector<int2> wmeta;  // [total_blocks * NW] {first chunk, chunk count}
  std::vector<int4> sell;
};
int plan_sell(const SegTable& tab, int NW, int LF, const std::vector<int32_t>& rp, const std::vector<int32_t>& col,
              SellTable* out);

// step.hip: the padded CSR
struct PaddedCsr {
  std::vector<int32_t> prp, pcol;
};
int plan_pcol(const std::vector<int32_t>& rp, const std::vector<int32_t>& col, PaddedCsr* out);

// tiles.hip: the hybrid step's dense blocks, work items and tail-first columns of rows [0, n_plan)
struct TileKnobs {
  int th = 96;        // entries that make a dense block (>= 1)
  int tile_max = 0;   // blocks per work item, <= 0: auto
  int rows = 128;     // rows per row block (64 or 128)
  int probe_tailwin = 0;
  bool fused_possible = false;  // the fused launch's tile shape can apply: its own item list
};
struct TileTables {
  std::vector<int32_t> bct, tcol, tsplit;
  std::vector<uint32_t> bmask;
  std::vector<int4> items, multi, fitems, fmulti;  // fitems empty: the fused launch walks items
  int32_t n_blocks = 0, n_slots = 0, n_fslots = 0;
  int64_t dense_nnz = 0;
  std::string text;
};
int plan_tiles(const std::vector<int32_t>& rp, const std::vector<int32_t>& col, int64_t n_plan, int64_t n_cols,
               int64_t col_limit, const TileKnobs& k, TileTables* out);

}  // namespace wg
