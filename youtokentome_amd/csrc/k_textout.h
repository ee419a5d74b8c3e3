// k_textout.h -- what the text-producing kernels of the k_encode.hip unit share (k_decode.h, k_subword.h, k_idtext.h, k_spans.h): the walk of a
// wavefront over its groups of sentences, the group's boundaries held a lane each, the LDS tile through which a wavefront writes its contiguous
// part of an output blob, and the host's group size and grid.  DESIGN.md "The tile writer" states the writer's protocol once; the comments on
// its members are the invariants each relies on.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "yttm_device.h"

namespace yttm {

// ---- the group walk ------------------------------------------------------------------------------------------------------------------------
// n_items in groups of `group` consecutive ones; wavefront w of the grid takes groups w, w + n_waves, ...: group g holds items [g0(), g1()).
struct WaveGroups {
  unsigned long long n_items, n_groups, n_waves, g;
  unsigned int group;
  __device__ WaveGroups(unsigned long long items, unsigned int per_group, int w)
      : n_items(items), n_groups((items + per_group - 1) / per_group), n_waves((unsigned long long)gridDim.x * NWAVES),
        g((unsigned long long)blockIdx.x * NWAVES + (unsigned long long)w), group(per_group) {}
  __device__ bool more() const { return g < n_groups; }
  __device__ void next() { g += n_waves; }
  __device__ unsigned long long g0() const { return g * group; }
  __device__ unsigned long long g1() const { return g0() + group < n_items ? g0() + group : n_items; }
};

// The boundaries off[g0 .. g1] of a group, lane j holding off[g0 + j]: item j of the group is [at(j), at(j + 1)).  A lane per boundary, so a
// group has at most LANE_GROUP_MAX items (the host's group size caps it there).
constexpr unsigned int LANE_GROUP_MAX = 63;
struct LaneBounds {
  unsigned long long mine;
  __device__ LaneBounds(const unsigned long long *off, unsigned long long g0, unsigned long long g1, uint32_t lane)
      : mine(g0 + lane <= g1 ? off[g0 + lane] : 0ull) {}
  __device__ unsigned long long at(int j) const { return uni64(__shfl(mine, j)); }
};

// ---- the tile writer -----------------------------------------------------------------------------------------------------------------------
constexpr int DEC_TILE = 2048;                // bytes of LDS staging per wavefront
constexpr int DEC_SEG = DEC_TILE - 16;        // most bytes staged at once: up to 15 bytes of an unfinished 16-byte unit stay in front of them
constexpr uint32_t SUB_FLUSH = DEC_TILE / 2;  // flush_if_due: the tile is flushed once it holds this much
static_assert(15 + DEC_SEG <= DEC_TILE, "a segment of a piece fits behind an unfinished unit");
static_assert(SUB_FLUSH + 64 + 1 <= (uint32_t)DEC_TILE, "a 64-byte step of a run and a space fit behind SUB_FLUSH - 1 staged bytes");

// The staged bytes mirror out[base .. base + fill): base is a multiple of 16; the first `head` bytes of the tile belong to the group before
// this one (another wavefront writes them) and are never stored.  All lanes of the wavefront call every member together.
class TileWriter {
  uint8_t *tile;
  uint8_t *out;
  unsigned long long base;
  uint32_t fill, head;
  const uint32_t lane;  // of the calling thread

  // Builds without hipcc only (the CPU emulator of tests/hipsim compiles the kernels with the host compiler): bytes staged past the tile's end land in the next
  // wavefront's tile and are read back from there, so no output shows them; the room rules of the members below are checked here instead.
  __device__ void check_room(uint32_t n) const {
#if !defined(__HIP__)  // (hipcc defines it in both of its passes)
    if (fill + n > (uint32_t)DEC_TILE) {
      fprintf(stderr, "TileWriter: %u bytes staged behind %u do not fit the tile\n", n, fill);
      abort();
    }
#endif
  }
  // end of a group: the unfinished unit is shared with the next group: bytes
  __device__ void flush_tail() {
    if (lane >= head && lane < fill) out[base + lane] = tile[lane];
    wave_sync();
  }

 public:
  // A writer over `lds_tile` (DEC_TILE bytes, 16-byte aligned, the wavefront's own); nothing is written before open().
  __device__ TileWriter(uint8_t *lds_tile, uint32_t lane_of_thread) : tile(lds_tile), out(nullptr), base(0), fill(0), head(0), lane(lane_of_thread) {}
  // The group's output starts at blob[cursor] (blob: 16-byte aligned).  The bytes of cursor's unit in front of it are the group before's:
  // they count as staged (head), so that every position keeps its place in its 16-byte unit, and are skipped by the stores.
  __device__ void open(uint8_t *blob, unsigned long long cursor) {
    out = blob;
    base = cursor & ~15ull;
    head = fill = (uint32_t)(cursor & 15ull);
  }
  // Do n more bytes fit?  Asked before every append whose caller cannot tell; after flush_units() fewer than 16 bytes are staged, so whatever
  // is at most DEC_SEG long fits then.
  __device__ bool fits(uint32_t n) const { return fill + n <= (uint32_t)DEC_TILE; }
  // A step's pieces, a lane each: the lane whose piece starts x bytes into the step writes it at at(x) (x from a wave scan of the lengths,
  // the step's total within fits()), then commit(total) makes the step's bytes part of the tile.
  __device__ uint8_t *at(uint32_t x) const { return tile + fill + x; }
  __device__ void commit(uint32_t total) {
    check_room(total);
    wave_sync();
    fill += total;
  }
  // stores every complete 16-byte unit; the rest (< 16 bytes) moves to the front of the tile
  __device__ void flush_units() {
    const uint32_t full = fill >> 4;
    if (!full) return;
    uint32_t u0 = 0;
    if (head) {  // the group's first unit is shared with the group before: bytes
      if (lane >= head && lane < 16u) out[base + lane] = tile[lane];
      u0 = 1;
      head = 0;
    }
    for (uint32_t u = u0 + lane; u < full; u += 64) *reinterpret_cast<uint4 *>(out + base + 16ull * u) = *reinterpret_cast<const uint4 *>(tile + 16u * u);
    const uint32_t rem = fill & 15u;
    const uint8_t v = lane < rem ? tile[16u * full + lane] : (uint8_t)0;
    wave_sync();
    if (lane < rem) tile[lane] = v;
    wave_sync();
    base += 16ull * full;
    fill = rem;
  }
  // The threshold flush of the appends that do not flush every time: behind it fewer than SUB_FLUSH bytes are staged, so a step of up to
  // DEC_TILE - SUB_FLUSH bytes fits without asking (the consumers' static_asserts name their steps).
  __device__ void flush_if_due() {
    if (fill >= SUB_FLUSH) flush_units();
  }
  // One byte, written by lane 0.
  __device__ void append_byte(uint8_t c) {
    if (!fits(1u)) flush_units();
    if (lane == 0) tile[fill] = c;
    commit(1u);
    flush_if_due();
  }
  // n <= 64 copies of one byte, a lane each, then flush_units().  Needs at most DEC_TILE - 64 staged bytes: true behind any flush.
  __device__ void append_run(uint8_t c, uint32_t n) {
    if (lane < n) tile[fill + lane] = c;
    commit(n);
    flush_units();
  }
  // One step of a filtered stream: the lanes with `keep` append byte() in lane order.  Needs fewer than SUB_FLUSH staged bytes (64 more fit)
  // and leaves it so.
  template <class F>
  __device__ void append_kept(bool keep, F &&byte) {
    const unsigned long long K = ballot_b(keep);
    if (keep) tile[fill + (uint32_t)__popcll(K & lanemask_lt())] = byte();
    commit((uint32_t)__popcll(K));
    flush_if_due();
  }
  // One piece of any length, copied by the whole wavefront in segments of DEC_SEG, each flushed: fewer than 16 bytes stay staged.
  __device__ void copy_piece(const uint8_t *src, uint32_t n_bytes) {
    for (uint32_t done = 0; done < n_bytes;) {
      const uint32_t n = n_bytes - done < (uint32_t)DEC_SEG ? n_bytes - done : (uint32_t)DEC_SEG;
      if (!fits(n)) flush_units();  // (an append in front left up to SUB_FLUSH bytes; now fewer than 16)
      for (uint32_t b = lane; b < n; b += 64) tile[fill + b] = src[done + b];
      commit(n);
      flush_units();
      done += n;
    }
  }
  // End of the group: every staged byte that is the group's own is stored.  Behind flush_units() fewer than 16 bytes remain, all of one unit
  // that the next group shares: flush_tail() stores them as bytes.
  __device__ void close() {
    flush_units();
    flush_tail();
  }
};

// ---- the host's side of the walk -----------------------------------------------------------------------------------------------------------
constexpr unsigned long long GRID_MAX = 256ull * 8;  // workgroups of a grid-stride launch: 8 for each of the 256 CUs
// workgroups for n_items, per_block to a workgroup
static inline dim3 grid_for(unsigned long long n_items, unsigned long long per_block) {
  const unsigned long long b = (n_items + per_block - 1) / per_block;
  return dim3((unsigned int)(b > GRID_MAX ? GRID_MAX : b));
}
// Items per group (n_items > 0, `total` units of work in all): about `target` units, in a large batch enough that a wavefront has a few groups,
// not thousands; within [1, cap].
static inline unsigned int group_size(unsigned long long n_items, unsigned long long total, unsigned long long target, unsigned long long cap) {
  const unsigned long long avg = total / n_items, many = n_items / (GRID_MAX * NWAVES * 4);
  unsigned long long grp = target / (avg ? avg : 1);
  if (grp < many) grp = many;
  return (unsigned int)(grp < 1 ? 1 : grp > cap ? cap : grp);
}
// workgroups for the walk of n_items in groups of `group`, a group to a wavefront
static inline dim3 grid_for_groups(unsigned long long n_items, unsigned int group) { return grid_for((n_items + group - 1) / group, NWAVES); }

}  // namespace yttm
