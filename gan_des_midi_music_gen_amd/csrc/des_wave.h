// What the one-wave-per-sample kernels of the batched simulator share (des_batch.hip: the logging kernel; des_stats.hip:
// the log-free statistics kernel): the workspace layout, the LDS block of one sample, and the prologue every lane takes
// part in -- parameters to LDS, routing tables (one node per lane), the checks of the batch entries and the seeder's
// draws (lane 0), init_genrand (one generator per lane) -- up to the point where lane 0 runs the chain, and the
// write-back of the global generator behind it; and the three node policies both files instantiate their kernel for
// (NormalOnly, AnyDist, AnyNode: the Dist of des::Sim, the LDS block beside Lds, its staging).  Device code only.
#pragma once
#include "gdm_common.h"
#include "des_sim.h"

#pragma clang fp contract(off)

namespace des_wave {

constexpr int kMaxDim = GDM_DES_BATCH_MAX_DIM;
#ifndef GDM_DES_LDS_GEN_DIM
#define GDM_DES_LDS_GEN_DIM 15        // (an experiment build may move it: 0 keeps every node generator in the workspace)
#endif
constexpr int kLdsGenDim = GDM_DES_LDS_GEN_DIM;

// per sample: node generators (unused when they fit LDS), routing tables, the FIFO rings of customer ids and -- the
// statistics kernel only -- the ring of their arrival times, slot for slot beside the ids
struct WsLayout {
  size_t keys, children, cdf, ring, atime, per_sample;
};
__host__ __device__ inline size_t align16(size_t n) { return (n + 15) & ~(size_t)15; }
__host__ __device__ inline WsLayout ws_layout(int dim, int max_queue_cap, bool with_atime) {
  WsLayout w;
  w.keys = 0;
  w.children = w.keys + align16((size_t)dim * DES_MT_N * 4);
  w.cdf = w.children + align16((size_t)dim * dim * 4);
  w.ring = w.cdf + align16((size_t)dim * dim * 8);
  w.atime = w.ring + align16((size_t)dim * max_queue_cap * 8);
  w.per_sample = w.atime + (with_atime ? align16((size_t)dim * max_queue_cap * 8) : 0);
  return w;
}
inline size_t lds_dyn_bytes(int dim) { return dim <= kLdsGenDim ? (size_t)dim * DES_MT_N * 4 : 0; }

// the static LDS of one sample: the event list, the per-node scalars, the global generator and the seeder
struct Lds {
  des::Ev heap[kMaxDim + 1];
  double loc[kMaxDim], scale[kMaxDim], gauss[kMaxDim + 2];
  uint32_t gkey[DES_MT_N], skey[DES_MT_N], node_seed[kMaxDim];
  int32_t qcap[kMaxDim], in_service[kMaxDim], qhead[kMaxDim], qlen[kMaxDim], nchild[kMaxDim];
  int32_t pos[kMaxDim + 2], has_gauss[kMaxDim + 2];
  uint8_t is_source[kMaxDim], bflags[kMaxDim];
  int ok;
};

// the kinds of one sample for the kernels over des::AnyDist (512 B), staged by every lane of the wave.  Before the
// prologue, whose first barrier orders it before any read.
struct DistLds {
  int32_t kind[kMaxDim];
};
__device__ inline void stage_dist(des::AnyDist& d, DistLds& n, const int32_t* __restrict__ kind, int dim, int b,
                                  int lane) {
  for (int i = lane; i < dim; i += GDM_WAVE) n.kind[i] = kind[(int64_t)b * dim + i];
  d.kind = n.kind;
}

// the kinds and the node state of one sample for the kernels over des::AnyNode (2 KB), and their staging by every lane
// of the wave: the kinds of sample b, no delayed departure, no departure scheduled yet.  Before the prologue, as above.
struct NetLds {
  double next_departure[kMaxDim];
  int32_t kind[kMaxDim], delayed[kMaxDim];
};
__device__ inline void stage_net(des::AnyNode& d, NetLds& n, const int32_t* __restrict__ kind, int dim, int b,
                                 int lane) {
  d.kind = n.kind;
  d.delayed = n.delayed;
  d.next_departure = n.next_departure;
  for (int i = lane; i < dim; i += GDM_WAVE) n.kind[i] = kind[(int64_t)b * dim + i];
  d.reset(dim, lane, GDM_WAVE);
}

// A node policy of the batch kernels, described once: the Dist it gives des::Sim, the LDS block it needs beside Lds,
// how every lane stages that block before the prologue, and whether its entries take a (B, dim) `kind` array at all
// (the kernels are instantiated per policy in des_batch.hip and des_stats.hip; NormalOnly ignores the pointer).
struct NoLds {};
struct NormalOnly {
  typedef des::NormalOnly Dist;
  typedef NoLds Block;
  static constexpr bool kHasKind = false;
  __device__ static void stage(Dist&, Block&, const int32_t*, int, int, int) {}
};
struct AnyDist {
  typedef des::AnyDist Dist;
  typedef DistLds Block;
  static constexpr bool kHasKind = true;
  __device__ static void stage(Dist& d, Block& n, const int32_t* __restrict__ kind, int dim, int b, int lane) {
    stage_dist(d, n, kind, dim, b, lane);
  }
};
struct AnyNode {
  typedef des::AnyNode Dist;
  typedef NetLds Block;
  static constexpr bool kHasKind = true;
  __device__ static void stage(Dist& d, Block& n, const int32_t* __restrict__ kind, int dim, int b, int lane) {
    stage_net(d, n, kind, dim, b, lane);
  }
};
constexpr size_t kMaxPolicyLds = sizeof(NetLds);        // the largest Block: what the kernels' LDS sums count
static_assert(sizeof(DistLds) <= kMaxPolicyLds, "kMaxPolicyLds is not the largest policy block");

// Every lane of the wave: binds the simulator's storage (dyn: the dynamic LDS, lds_dyn_bytes(dim); ws: the sample's
// workspace), stages sample b and leaves the node generators seeded.  Returns whether the spec passed the checks of
// the batch entries (uniform over the wave); a refused sample runs nothing.  s.out / s.out_cap / s.max_records /
// s.stats are the caller's.
template <class SimT>
__device__ inline bool prologue(SimT& s, Lds& l, unsigned char* dyn, unsigned char* ws, const WsLayout& w, int b,
                                int lane, const double* __restrict__ adj, int dim, const double* __restrict__ loc,
                                const double* __restrict__ scale, const int32_t* __restrict__ queue_cap,
                                const int64_t* __restrict__ seed, int max_queue_cap, int64_t max_events,
                                const uint32_t* __restrict__ mt_key, const int32_t* __restrict__ mt_pos,
                                const int32_t* __restrict__ mt_has_gauss, const double* __restrict__ mt_gauss) {
  s.dim = dim;
  s.loc = l.loc;
  s.scale = l.scale;
  s.qcap = l.qcap;
  s.is_source = l.is_source;
  s.in_service = l.in_service;
  s.qhead = l.qhead;
  s.qlen = l.qlen;
  s.nchild = l.nchild;
  s.bflags = l.bflags;
  s.children = reinterpret_cast<int32_t*>(ws + w.children);
  s.cdf = reinterpret_cast<double*>(ws + w.cdf);
  s.ring = reinterpret_cast<int64_t*>(ws + w.ring);
  s.ring_stride = max_queue_cap;
  s.node_keys = dim <= kLdsGenDim ? reinterpret_cast<uint32_t*>(dyn) : reinterpret_cast<uint32_t*>(ws + w.keys);
  s.global_key = l.gkey;
  s.seeder_key = l.skey;
  s.pos = l.pos;
  s.has_gauss = l.has_gauss;
  s.gauss = l.gauss;
  s.heap = l.heap;
  s.heap_cap = dim + 1;
  s.draws_left = (int64_t)DES_DRAW_FACTOR * (max_events + dim + 1);
  s.reset();

  // ---- all lanes: parameters to LDS, the global generator's words
  for (int i = lane; i < dim; i += GDM_WAVE) {
    l.loc[i] = loc[(int64_t)b * dim + i];
    l.scale[i] = scale[(int64_t)b * dim + i];
    l.qcap[i] = queue_cap[(int64_t)b * dim + i];
  }
  for (int i = lane; i < DES_MT_N; i += GDM_WAVE) l.gkey[i] = mt_key[(int64_t)b * DES_MT_N + i];
  __syncthreads();
  // ---- one node per lane: source flags and routing tables
  s.setup_nodes(adj + (int64_t)b * dim * dim, lane, GDM_WAVE);
  __syncthreads();
  // ---- lane 0: the checks of the batch entries, then the seeder's draws
  if (lane == 0) {
    const int64_t sd = seed[b];
    const int32_t p0 = mt_pos[b];
    const int ok = s.spec_ok(sd, p0) ? 1 : 0;
    l.ok = ok;
    if (ok) {
      s.draw_node_seeds((uint32_t)sd, l.node_seed);
      l.pos[dim] = p0;
      l.has_gauss[dim] = mt_has_gauss[b];
      l.gauss[dim] = mt_gauss[b];
    }
  }
  __syncthreads();
  const bool ok = l.ok != 0;
  // ---- one generator per lane: init_genrand
  if (ok) s.seed_nodes(l.node_seed, lane, GDM_WAVE);
  __syncthreads();
  return ok;
}

// lane 0, after the chain: the global generator's scalars; all lanes, after a barrier: its words
__device__ inline void store_generator_scalars(const Lds& l, int dim, int b, int32_t* __restrict__ mt_pos,
                                               int32_t* __restrict__ mt_has_gauss, double* __restrict__ mt_gauss) {
  mt_pos[b] = l.pos[dim];
  mt_has_gauss[b] = l.has_gauss[dim];
  mt_gauss[b] = l.gauss[dim];
}
__device__ inline void store_generator_words(const Lds& l, int b, int lane, uint32_t* __restrict__ mt_key) {
  for (int i = lane; i < DES_MT_N; i += GDM_WAVE) mt_key[(int64_t)b * DES_MT_N + i] = l.gkey[i];
}

}  // namespace des_wave
