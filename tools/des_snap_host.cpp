// The snapshot policy des::SnapStats of csrc/des_sim.h (the statistics at S customer counts of one run) over des::AnyNode
// as a stand-alone host program, for a sanitizer build (no HIP, nothing loaded into Python): like tools/des_net_host.cpp
// with EXACTLY sized heap buffers -- S checkpoints, snapshot rows of S * dim entries, S histograms of dim * (stride + 1)
// columns, stride the case's largest queue capacity, and the rest as tools/des_stats_host.cpp sizes it -- so that an
// index des_sim.h fails to check shows as a heap-buffer-overflow instead of landing in slack.
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I gan_des_midi_music_gen_amd/csrc tools/des_snap_host.cpp -o des_snap_host
//   ./des_snap_host cases.bin snaps.bin
//
// Input (little endian, packed):  int32 n_cases, then per case
//   int32 dim, int32 has_gauss, int32 pos, int32 n_snap, int64 seed, int64 max_events, double gauss,
//   double adj[dim * dim], double loc[dim], double scale[dim], int32 kind[dim], int32 qcap[dim], uint32 key[624],
//   int64 checkpoints[n_snap]
// Output: per case  int32 stop_reason (the run's), int32 has_gauss, int32 pos, int32 stride, double gauss, then with
//   S = n_snap: int32 stop[S], int64 total_customers[S], events[S], n_records[S], double clock[S], end_time[S],
//   int64 served[S * dim], reneges[S * dim], generated[S * dim], int32 max_queue[S * dim], double
//   time_in_service[S * dim], time_in_queue[S * dim], queue_area[S * dim], arrival_time[S * dim],
//   double queue_time[S * dim * (stride + 1)], uint32 key[624]
// The checkpoints of a case ascend strictly from >= 1 (the library's entry refuses any other row before anything runs;
// this program trusts its input).  tests/test_des_snap.py writes cases in this form and compares with
// gdm_des_stats_batch_snap_host(math = 1).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "des_sim.h"

namespace {

template <class T>
void get(std::FILE* f, T* p, size_t n) {
  if (n && std::fread(p, sizeof(T), n, f) != n) {
    std::fprintf(stderr, "des_snap_host: short read\n");
    std::exit(2);
  }
}
template <class T>
void put(std::FILE* f, const std::vector<T>& v) {
  if (!v.empty() && std::fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) {
    std::fprintf(stderr, "des_snap_host: short write\n");
    std::exit(2);
  }
}

struct Header {
  int32_t dim, has_gauss, pos, n_snap;
  int64_t seed, max_events;
  double gauss;
};

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) {
    std::fprintf(stderr, "usage: %s cases.bin snaps.bin\n", argv[0]);
    return 2;
  }
  std::FILE* in = std::fopen(argv[1], "rb");
  std::FILE* outf = std::fopen(argv[2], "wb");
  if (!in || !outf) {
    std::fprintf(stderr, "des_snap_host: cannot open files\n");
    return 2;
  }
  int32_t n_cases = 0;
  get(in, &n_cases, 1);
  for (int32_t c = 0; c < n_cases; ++c) {
    Header h;
    get(in, &h, 1);
    const int dim = h.dim, S = h.n_snap;
    if (dim < 1 || dim > 4096 || S < 1 || S > 256) {
      std::fprintf(stderr, "des_snap_host: bad case header\n");
      return 2;
    }
    const size_t d = (size_t)dim, n = (size_t)S;
    std::vector<double> adj(d * d), loc(d), scale(d);
    std::vector<int32_t> kind(d), qcap(d);
    std::vector<uint32_t> global_key(DES_MT_N);
    std::vector<int64_t> checkpoints(n);
    get(in, adj.data(), d * d);
    get(in, loc.data(), d);
    get(in, scale.data(), d);
    get(in, kind.data(), d);
    get(in, qcap.data(), d);
    get(in, global_key.data(), DES_MT_N);
    get(in, checkpoints.data(), n);
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
    // the running accumulators: scratch
    std::vector<int64_t> served(d), reneges(d), generated(d);
    std::vector<int32_t> max_queue(d), delayed(d);
    std::vector<double> tis(d), tiq(d), area(d), arrival(d), last_change(d), atime(d * (size_t)stride), next_departure(d);
    // the snapshots
    std::vector<int32_t> o_stop(n), o_max_queue(n * d);
    std::vector<int64_t> o_total(n), o_events(n), o_records(n), o_served(n * d), o_reneges(n * d), o_generated(n * d);
    std::vector<double> o_clock(n), o_end(n), o_tis(n * d), o_tiq(n * d), o_area(n * d), o_arrival(n * d),
        o_queue_time(n * d * hs, 0.0);

    des::Sim<des::MathPortable, des::OutNone, des::SnapStats, des::AnyNode> s;
    s.dist.kind = kind.data();
    s.dist.delayed = delayed.data();
    s.dist.next_departure = next_departure.data();
    s.dist.reset(dim, 0, 1);
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
    des::SnapStats& st = s.stats;
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
    st.ring_stride = stride;
    st.hist_stride = (int64_t)hs;
    st.snap_customers = checkpoints.data();
    st.n_snap = S;
    st.dim = dim;
    st.is_source = is_source.data();
    st.next = 0;
    st.o = des::SnapOut{o_served.data(), o_reneges.data(), o_generated.data(), o_max_queue.data(), o_tis.data(),
                        o_tiq.data(),    o_area.data(),    o_arrival.data(),   o_clock.data(),     o_end.data(),
                        o_total.data(),  o_events.data(),  o_records.data(),   o_stop.data(),      o_queue_time.data()};
    st.queue_time = o_queue_time.data() + (n - 1) * d * hs;          // the running histogram: the last snapshot's slot
    st.reset(dim, 0, 1);

    int32_t reason = DES_STOP_ERROR;
    pos[d] = h.pos;
    has_gauss[d] = h.has_gauss;
    gauss[d] = h.gauss;
    if (s.spec_ok(h.seed, h.pos)) {                       // the order of the batch entries (des_core.hip)
      s.setup_nodes(adj.data(), 0, 1);
      s.draw_node_seeds((uint32_t)h.seed, node_seed.data());
      s.seed_nodes(node_seed.data(), 0, 1);
      reason = s.run(checkpoints[n - 1], h.max_events);
    }
    const bool keep = reason != DES_STOP_ERROR;
    if (!keep) {
      global_key = key0;
      pos[d] = h.pos;
      has_gauss[d] = h.has_gauss;
      gauss[d] = h.gauss;
    }
    st.flush(reason, s.total_customers, s.clock, s.n_out);
    const std::vector<int32_t> head = {reason, has_gauss[d], pos[d], (int32_t)stride};
    put(outf, head);
    put(outf, std::vector<double>{gauss[d]});
    put(outf, o_stop);
    put(outf, o_total);
    put(outf, o_events);
    put(outf, o_records);
    put(outf, o_clock);
    put(outf, o_end);
    put(outf, o_served);
    put(outf, o_reneges);
    put(outf, o_generated);
    put(outf, o_max_queue);
    put(outf, o_tis);
    put(outf, o_tiq);
    put(outf, o_area);
    put(outf, o_arrival);
    put(outf, o_queue_time);
    put(outf, global_key);
  }
  std::fclose(in);
  if (std::fclose(outf) != 0) return 2;
  return 0;
}
