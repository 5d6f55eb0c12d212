// plan_tables.h -- the tables of a plan as both builders write them (the host builder of plan_host.h, the kernels of
// plan_kernels.hip.h), as the counting kernels of pc_kernels.hip.h read them and as pc_plan_table hands them out, byte
// for byte.  Plain C++: no HIP, so that the host builder can be compiled and tested on a machine without a GPU.
#pragma once
#include <stdint.h>

#include "../../include/plastid_counts.h"   // (by its place in the tree: the host headers that include this file are compiled with this directory alone on the include path)

namespace pc {

constexpr int kWave = 64;
constexpr int kGatherChunk = 1024;
constexpr int kStreamMaxLen = 255;        // aligned lengths the 4-byte record stream can carry
constexpr int kOpStage = 32;              // output pieces of a window that k_hist_point stages in LDS ahead of its epilogue

// strand modes of a query interval
//   0: '+'  keeps forward reads, forward index rule
//   1: '-'  keeps reverse reads, reverse index rule
//   2: '.'  keeps all reads,     forward index rule  (map_factories.pyx:345-346: only '-' flips)
//   3: all reads, reverse index rule (direct map-factory call on a '-' segment, no strand filter)
constexpr int kModes = 4;

inline int mode_of(uint8_t strand) {
    const bool nofilter = strand & PC_STRAND_NOFILTER;
    const int s = strand & 3;
    if (s == PC_STRAND_REV) return nofilter ? 3 : 1;
    if (s == PC_STRAND_FWD) return nofilter ? 2 : 0;
    return 2; // '.' and undefined: all reads, forward rule
}

struct Tile {
    int32_t tid;
    int32_t win_start;
    uint32_t piece_begin; // island pieces (histogram coordinates)
    uint32_t piece_end;
    uint32_t mode_mask;
    uint32_t op_begin;    // output pieces (segment slices in the caller's layout)
    uint32_t op_end;
    uint16_t span_lo;     // queried positions of the window all lie in [span_lo, span_hi) (window-relative)
    uint16_t span_hi;
};

// A queried segment cut at the tile grid, with its place in the caller's output buffer:
// position start+i, row r  ->  out[out_off + step*i + r*row_stride]
struct OutPiece {
    int64_t out_off;
    int64_t row_stride;
    int64_t hist_off; // same positions in the compact histogram (used when a tile is split)
    int32_t start;
    int32_t len;
    int32_t mode;
    int32_t step;
};

struct Piece {
    int64_t hist_off;
    int32_t start;
    int32_t len;
    int32_t mode;
    int32_t pad;
};

struct CenterChunk {
    int64_t hist_off;
    int32_t tid;
    int32_t start;
    int32_t len;
    int32_t mode;
    uint32_t op_begin, op_end;   // output pieces of the chunk's window (Tile::op_begin / op_end): where its sums go
};

struct GatherSeg {
    int64_t out_off;
    int64_t row_stride;
    int64_t hist_off; // hist index of position (start + clip_lo); -1: all zero
    int64_t len;
    int64_t clip_lo, clip_hi;
    int64_t start;    // genomic coordinate of the segment's first position
    int32_t step;
    int32_t pad;
};

struct GatherChunk {
    uint32_t seg;
    uint32_t chunk;
};

// (no padding anywhere: the tables of the two builders are compared as bytes)
static_assert(sizeof(Tile) == 32, "Tile is 32 bytes in HBM and in pc_plan_table");
static_assert(sizeof(OutPiece) == 40, "OutPiece is 40 bytes in HBM and in pc_plan_table");
static_assert(sizeof(Piece) == 24, "Piece is 24 bytes in HBM and in pc_plan_table");
static_assert(sizeof(CenterChunk) == 32, "CenterChunk is 32 bytes in HBM");
static_assert(sizeof(GatherSeg) == 64, "GatherSeg is 64 bytes in HBM and in pc_plan_table");
static_assert(sizeof(GatherChunk) == 8, "GatherChunk is 8 bytes in HBM");

} // namespace pc
