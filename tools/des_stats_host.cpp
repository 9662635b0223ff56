// The statistics mode of csrc/des_sim.h as a stand-alone host program, for a sanitizer build (no HIP, nothing loaded
// into Python): des::Sim<MathPortable, OutNone, NodeStats> on cases read from a flat binary file, with EXACTLY sized heap
// buffers -- an event list of dim + 1, an id ring and an arrival-time ring whose stride is the case's largest queue
// capacity, a histogram of stride + 1 columns, accumulators of dim entries -- so that an index des_sim.h fails to check
// shows as a heap-buffer-overflow instead of landing in slack.
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I gan_des_midi_music_gen_amd/csrc tools/des_stats_host.cpp -o des_stats_host
//   ./des_stats_host cases.bin stats.bin
//
// Input (little endian, packed):  int32 n_cases, then per case
//   int32 dim, int32 has_gauss, int32 pos, int32 pad, int64 seed, int64 customers, int64 max_events, double gauss,
//   double adj[dim * dim], double loc[dim], double scale[dim], int32 qcap[dim], uint32 key[624]
// Output: per case  int32 stop_reason, int32 has_gauss, int32 pos, int32 stride, int64 total_customers, int64 events,
//   int64 n_records, double gauss, double clock, double end_time, int64 served[dim], reneges[dim], generated[dim],
//   int32 max_queue[dim], double time_in_service[dim], time_in_queue[dim], queue_area[dim], arrival_time[dim],
//   double queue_time[dim * (stride + 1)], uint32 key[624]
// A case that stops with DES_STOP_ERROR gives zeros and the generator state it came with, as the batch entries do.
// tests/test_des_stats.py writes corpus cases in this form and compares with gdm_des_stats_batch_host(math = 1).
//
// With DES_HOST_WITH_KIND defined (tools/des_dist_host.cpp does, and includes this file) the simulator is
// des::Sim<MathPortable, OutNone, NodeStats, AnyDist> and every case carries int32 kind[dim] between scale and qcap:
// an exactly sized array, so a kind read past the case's nodes shows too.  With DES_HOST_WITH_NODES as well
// (tools/des_net_host.cpp) the policy is des::AnyNode -- kinds 'queue' and 'branch' too -- with its two per-node arrays,
// delayed departures and next departure times, exactly sized like the rest.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "des_sim.h"

namespace {

template <class T>
void get(std::FILE* f, T* p, size_t n) {
  if (n && std::fread(p, sizeof(T), n, f) != n) {
    std::fprintf(stderr, "des_stats_host: short read\n");
    std::exit(2);
  }
}
template <class T>
void put(std::FILE* f, const T* p, size_t n) {
  if (n && std::fwrite(p, sizeof(T), n, f) != n) {
    std::fprintf(stderr, "des_stats_host: short write\n");
    std::exit(2);
  }
}

struct Header {
  int32_t dim, has_gauss, pos, pad;
  int64_t seed, customers, max_events;
  double gauss;
};

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) {
    std::fprintf(stderr, "usage: %s cases.bin stats.bin\n", argv[0]);
    return 2;
  }
  std::FILE* in = std::fopen(argv[1], "rb");
  std::FILE* outf = std::fopen(argv[2], "wb");
  if (!in || !outf) {
    std::fprintf(stderr, "des_stats_host: cannot open files\n");
    return 2;
  }
  int32_t n_cases = 0;
  get(in, &n_cases, 1);
  for (int32_t c = 0; c < n_cases; ++c) {
    Header h;
    get(in, &h, 1);
    const int dim = h.dim;
    if (dim < 1 || dim > 4096) {
      std::fprintf(stderr, "des_stats_host: bad case header\n");
      return 2;
    }
    const size_t d = (size_t)dim;
    std::vector<double> adj(d * d), loc(d), scale(d);
    std::vector<int32_t> qcap(d);
    std::vector<uint32_t> global_key(DES_MT_N);
    get(in, adj.data(), d * d);
    get(in, loc.data(), d);
    get(in, scale.data(), d);
#ifdef DES_HOST_WITH_KIND
    std::vector<int32_t> kind(d);
    get(in, kind.data(), d);
#endif
    get(in, qcap.data(), d);
    get(in, global_key.data(), DES_MT_N);
    const std::vector<uint32_t> key0 = global_key;
    int64_t stride = 0;                                   // the largest capacity: not one slot more
    for (int i = 0; i < dim; ++i) stride = qcap[i] > stride ? qcap[i] : stride;
    const size_t hs = (size_t)stride + 1;

    std::vector<uint8_t> is_source(d), bflags(d);
    std::vector<int32_t> in_service(d), qhead(d), qlen(d), nchild(d), children(d * d), pos(d + 2), has_gauss(d + 2);
    std::vector<double> cdf(d * d), gauss(d + 2);
    std::vector<int64_t> ring(d * (size_t)stride);
    std::vector<uint32_t> node_keys(d * DES_MT_N), seeder_key(DES_MT_N), node_seed(d);
    std::vector<des::Ev> heap(d + 1);
    std::vector<int64_t> served(d), reneges(d), generated(d);
    std::vector<int32_t> max_queue(d);
    std::vector<double> tis(d), tiq(d), area(d), arrival(d), last_change(d), atime(d * (size_t)stride),
        queue_time(d * hs, 0.0);

#if defined(DES_HOST_WITH_NODES)
    std::vector<int32_t> delayed(d);
    std::vector<double> next_departure(d);
    des::Sim<des::MathPortable, des::OutNone, des::NodeStats, des::AnyNode> s;
    s.dist.kind = kind.data();
    s.dist.delayed = delayed.data();
    s.dist.next_departure = next_departure.data();
    s.dist.reset(dim, 0, 1);
#elif defined(DES_HOST_WITH_KIND)
    des::Sim<des::MathPortable, des::OutNone, des::NodeStats, des::AnyDist> s;
    s.dist.kind = kind.data();
#else
    des::Sim<des::MathPortable, des::OutNone, des::NodeStats> s;
#endif
    s.dim = dim;
    s.loc = loc.data();
    s.scale = scale.data();
    s.qcap = qcap.data();
    s.is_source = is_source.data();
    s.in_service = in_service.data();
    s.qhead = qhead.data();
    s.qlen = qlen.data();
    s.nchild = nchild.data();
    s.bflags = bflags.data();
    s.children = children.data();
    s.cdf = cdf.data();
    s.ring = ring.data();
    s.ring_stride = stride;
    s.node_keys = node_keys.data();
    s.global_key = global_key.data();
    s.seeder_key = seeder_key.data();
    s.pos = pos.data();
    s.has_gauss = has_gauss.data();
    s.gauss = gauss.data();
    s.heap = heap.data();
    s.heap_cap = dim + 1;
    s.out = des::OutNone{};
    s.out_cap = INT64_MAX;
    s.max_records = 0;
    s.draws_left = (int64_t)DES_DRAW_FACTOR * (h.max_events + dim + 1);
    s.reset();
    des::NodeStats& st = s.stats;
    st.served = served.data();
    st.reneges = reneges.data();
    st.generated = generated.data();
    st.max_queue = max_queue.data();
    st.time_in_service = tis.data();
    st.time_in_queue = tiq.data();
    st.queue_area = area.data();
    st.arrival_time = arrival.data();
    st.last_change = last_change.data();
    st.atime = atime.data();
    st.queue_time = queue_time.data();
    st.ring_stride = stride;
    st.hist_stride = (int64_t)hs;
    st.reset(dim, 0, 1);

    int32_t reason = DES_STOP_ERROR;
    pos[d] = h.pos;
    has_gauss[d] = h.has_gauss;
    gauss[d] = h.gauss;
    if (s.spec_ok(h.seed, h.pos)) {                       // the order of the batch entries (des_core.hip, des_stats.hip)
      s.setup_nodes(adj.data(), 0, 1);
      s.draw_node_seeds((uint32_t)h.seed, node_seed.data());
      s.seed_nodes(node_seed.data(), 0, 1);
      reason = s.run(h.customers, h.max_events);
    }
    const bool keep = reason != DES_STOP_ERROR;
    if (!keep) {
      st.reset(dim, 0, 1);
      queue_time.assign(d * hs, 0.0);
      global_key = key0;
      pos[d] = h.pos;
      has_gauss[d] = h.has_gauss;
      gauss[d] = h.gauss;
    }
    const int32_t head[4] = {reason, has_gauss[d], pos[d], (int32_t)stride};
    const int64_t counts[3] = {keep ? s.total_customers : 0, keep ? st.events : 0, keep ? s.n_out : 0};
    const double times[3] = {gauss[d], keep ? s.clock : 0.0, keep ? st.end_time : 0.0};
    put(outf, head, 4);
    put(outf, counts, 3);
    put(outf, times, 3);
    put(outf, served.data(), d);
    put(outf, reneges.data(), d);
    put(outf, generated.data(), d);
    put(outf, max_queue.data(), d);
    put(outf, tis.data(), d);
    put(outf, tiq.data(), d);
    put(outf, area.data(), d);
    put(outf, arrival.data(), d);
    put(outf, queue_time.data(), d * hs);
    put(outf, global_key.data(), DES_MT_N);
  }
  std::fclose(in);
  if (std::fclose(outf) != 0) return 2;
  return 0;
}
