// The event logic of csrc/des_sim.h as a stand-alone host program, for a sanitizer build (no HIP, nothing loaded into
// Python): des::Sim<MathPortable, OutSoa> on cases read from a flat binary file, with EXACTLY sized heap buffers -- an
// event list of dim + 1, a ring stride equal to the case's largest queue capacity, record arrays of the expected length
// -- so that an index des_sim.h fails to check shows as a heap-buffer-overflow instead of landing in slack.
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I gan_des_midi_music_gen_amd/csrc tools/des_corpus_host.cpp -o des_corpus_host
//   ./des_corpus_host cases.bin records.bin
//
// Input (little endian, packed):  int32 n_cases, then per case
//   int32 dim, int32 has_gauss, int32 pos, int32 pad, int64 seed, int64 customers, int64 max_events, int64 out_len,
//   double gauss, double adj[dim * dim], double loc[dim], double scale[dim], int32 qcap[dim], uint32 key[624]
// Output: per case  int32 stop_reason, int32 has_gauss, int32 pos, int32 overflow, int64 n_out, int64 n_stored,
//   double gauss, double value[n_stored], int64 event_id[n_stored], int32 node[n_stored], int32 kind[n_stored],
//   uint32 key[624]        (n_stored = min(n_out, out_len))
// tests/test_des_corpus.py writes the corpus of tests/golden/des_corpus.npz in this form and compares the records with
// gdm_des_run_batch_host(math = 1).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "des_sim.h"

namespace {

template <class T>
void get(std::FILE* f, T* p, size_t n) {
  if (n && std::fread(p, sizeof(T), n, f) != n) {
    std::fprintf(stderr, "des_corpus_host: short read\n");
    std::exit(2);
  }
}
template <class T>
void put(std::FILE* f, const T* p, size_t n) {
  if (n && std::fwrite(p, sizeof(T), n, f) != n) {
    std::fprintf(stderr, "des_corpus_host: short write\n");
    std::exit(2);
  }
}

struct Header {
  int32_t dim, has_gauss, pos, pad;
  int64_t seed, customers, max_events, out_len;
  double gauss;
};

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) {
    std::fprintf(stderr, "usage: %s cases.bin records.bin\n", argv[0]);
    return 2;
  }
  std::FILE* in = std::fopen(argv[1], "rb");
  std::FILE* outf = std::fopen(argv[2], "wb");
  if (!in || !outf) {
    std::fprintf(stderr, "des_corpus_host: cannot open files\n");
    return 2;
  }
  int32_t n_cases = 0;
  get(in, &n_cases, 1);
  for (int32_t c = 0; c < n_cases; ++c) {
    Header h;
    get(in, &h, 1);
    const int dim = h.dim;
    if (dim < 1 || dim > 4096 || h.out_len < 0 || h.out_len > (1 << 24)) {
      std::fprintf(stderr, "des_corpus_host: bad case header\n");
      return 2;
    }
    const size_t d = (size_t)dim;
    std::vector<double> adj(d * d), loc(d), scale(d);
    std::vector<int32_t> qcap(d);
    std::vector<uint32_t> global_key(DES_MT_N);
    get(in, adj.data(), d * d);
    get(in, loc.data(), d);
    get(in, scale.data(), d);
    get(in, qcap.data(), d);
    get(in, global_key.data(), DES_MT_N);
    int64_t stride = 0;                                   // the largest capacity: not one slot more
    for (int i = 0; i < dim; ++i) stride = qcap[i] > stride ? qcap[i] : stride;

    std::vector<uint8_t> is_source(d), bflags(d);
    std::vector<int32_t> in_service(d), qhead(d), qlen(d), nchild(d), children(d * d), pos(d + 2), has_gauss(d + 2);
    std::vector<double> cdf(d * d), gauss(d + 2);
    std::vector<int64_t> ring(d * (size_t)stride);
    std::vector<uint32_t> node_keys(d * DES_MT_N), seeder_key(DES_MT_N), node_seed(d);
    std::vector<des::Ev> heap(d + 1);
    const size_t n_rec = (size_t)h.out_len;
    std::vector<double> value(n_rec);
    std::vector<int64_t> event_id(n_rec);
    std::vector<int32_t> node(n_rec), kind(n_rec);

    des::Sim<des::MathPortable, des::OutSoa> s;
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
    s.out = des::OutSoa{value.data(), event_id.data(), node.data(), kind.data()};
    s.out_cap = h.out_len;
    s.max_records = 0;
    s.draws_left = (int64_t)DES_DRAW_FACTOR * (h.max_events + dim + 1);
    s.reset();

    int32_t reason = DES_STOP_ERROR;
    if (s.spec_ok(h.seed, h.pos)) {                       // the order of the batch entries (des_core.hip, des_batch.hip)
      s.setup_nodes(adj.data(), 0, 1);
      s.draw_node_seeds((uint32_t)h.seed, node_seed.data());
      s.seed_nodes(node_seed.data(), 0, 1);
      pos[d] = h.pos;
      has_gauss[d] = h.has_gauss;
      gauss[d] = h.gauss;
      reason = s.run(h.customers, h.max_events);
    } else {
      pos[d] = h.pos;
      has_gauss[d] = h.has_gauss;
      gauss[d] = h.gauss;
    }
    const int32_t head[4] = {reason, has_gauss[d], pos[d], s.overflow ? 1 : 0};
    const int64_t n_stored = s.n_out < h.out_len ? s.n_out : h.out_len;
    const int64_t counts[2] = {s.n_out, n_stored};
    put(outf, head, 4);
    put(outf, counts, 2);
    put(outf, &gauss[d], 1);
    put(outf, value.data(), (size_t)n_stored);
    put(outf, event_id.data(), (size_t)n_stored);
    put(outf, node.data(), (size_t)n_stored);
    put(outf, kind.data(), (size_t)n_stored);
    put(outf, global_key.data(), DES_MT_N);
  }
  std::fclose(in);
  if (std::fclose(outf) != 0) return 2;
  return 0;
}
