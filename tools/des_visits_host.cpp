// The visit walk of csrc/des_visits.h -- what gdm_des_log_visits_host runs per sample -- as a stand-alone host program
// for a sanitizer build (no HIP, nothing loaded into Python).  Every buffer is EXACTLY sized: the record arrays of
// exactly the log's length, the scratch table of exactly des_visits::scratch_entries entries, and, after a first walk
// that only counts, table columns of exactly the counted rows, each its own allocation -- so that an index the walk
// fails to check shows as a heap-buffer-overflow instead of landing in slack.
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I gan_des_midi_music_gen_amd/csrc tools/des_visits_host.cpp -o des_visits_host
//   ./des_visits_host logs.bin tables.bin
//
// Input (little endian, packed):  int32 n_cases, then per case
//   int32 dim, int32 zero, int64 n, double value[n], int64 event_id[n], int32 node[n], int32 kind[n]
// Output: per case  int32 status, int32 zero, int64 n_visits, int64 n_customers, then the columns in the order of
//   des_visits::Visits (int32 x 3, int64 x 7, double x 5; n_visits entries each) and of des_visits::Customers (int64 x 2,
//   int32 x 2, double x 4; n_customers entries each).
// tests/test_des_visits.py writes logs in this form and compares with gdm_des_log_visits_host.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "des_visits.h"

namespace {

template <class T>
void get(std::FILE* f, T* p, size_t n) {
  if (n && std::fread(p, sizeof(T), n, f) != n) {
    std::fprintf(stderr, "des_visits_host: short read\n");
    std::exit(2);
  }
}
template <class T>
void put(std::FILE* f, const std::vector<T>& v) {
  if (!v.empty() && std::fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) {
    std::fprintf(stderr, "des_visits_host: short write\n");
    std::exit(2);
  }
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) {
    std::fprintf(stderr, "usage: %s logs.bin tables.bin\n", argv[0]);
    return 2;
  }
  std::FILE* in = std::fopen(argv[1], "rb");
  std::FILE* outf = std::fopen(argv[2], "wb");
  if (!in || !outf) {
    std::fprintf(stderr, "des_visits_host: cannot open files\n");
    return 2;
  }
  int32_t n_cases = 0;
  get(in, &n_cases, 1);
  for (int32_t ci = 0; ci < n_cases; ++ci) {
    int32_t head[2];
    int64_t n = 0;
    get(in, head, 2);
    get(in, &n, 1);
    const int dim = head[0];
    if (dim < 1 || dim > 4096 || n < 0 || n > ((int64_t)1 << 30)) {
      std::fprintf(stderr, "des_visits_host: bad case header\n");
      return 2;
    }
    std::vector<double> value((size_t)n);
    std::vector<int64_t> event_id((size_t)n);
    std::vector<int32_t> node((size_t)n), kind((size_t)n);
    get(in, value.data(), (size_t)n);
    get(in, event_id.data(), (size_t)n);
    get(in, node.data(), (size_t)n);
    get(in, kind.data(), (size_t)n);

    std::vector<des_visits::Open> open((size_t)des_visits::scratch_entries(n, dim));
    int64_t nv = 0, nc = 0;
    int status = 0;
    des_visits::sample_walk(value.data(), event_id.data(), node.data(), kind.data(), 0, n, dim, open.data(), nullptr,
                            nullptr, &nv, &nc, &status);
    std::vector<int32_t> v32[3], c32[2];
    std::vector<int64_t> v64[7], c64[2];
    std::vector<double> vf[5], cf[4];
    for (auto& c : v32) c.resize((size_t)nv);
    for (auto& c : v64) c.resize((size_t)nv);
    for (auto& c : vf) c.resize((size_t)nv);
    for (auto& c : c32) c.resize((size_t)nc);
    for (auto& c : c64) c.resize((size_t)nc);
    for (auto& c : cf) c.resize((size_t)nc);
    if (status == 0) {
      const des_visits::Visits vis{v32[0].data(), v32[1].data(), v32[2].data(), v64[0].data(), v64[1].data(),
                                   v64[2].data(), v64[3].data(), v64[4].data(), v64[5].data(), v64[6].data(),
                                   vf[0].data(),  vf[1].data(),  vf[2].data(),  vf[3].data(),  vf[4].data()};
      const des_visits::Customers cust{c64[0].data(), c64[1].data(), c32[0].data(), c32[1].data(),
                                       cf[0].data(),  cf[1].data(),  cf[2].data(),  cf[3].data()};
      int64_t nv2 = 0, nc2 = 0;
      int status2 = 0;
      des_visits::sample_walk(value.data(), event_id.data(), node.data(), kind.data(), 0, n, dim, open.data(), &vis,
                              &cust, &nv2, &nc2, &status2);
      if (nv2 != nv || nc2 != nc || status2 != 0) {
        std::fprintf(stderr, "des_visits_host: two walks over one log differ\n");
        return 3;
      }
    }
    const int32_t out_head[2] = {status, 0};
    const int64_t counts[2] = {nv, nc};
    if (std::fwrite(out_head, sizeof(int32_t), 2, outf) != 2 || std::fwrite(counts, sizeof(int64_t), 2, outf) != 2) return 2;
    for (auto& c : v32) put(outf, c);
    for (auto& c : v64) put(outf, c);
    for (auto& c : vf) put(outf, c);
    for (auto& c : c64) put(outf, c);
    for (auto& c : c32) put(outf, c);
    for (auto& c : cf) put(outf, c);
  }
  std::fclose(in);
  if (std::fclose(outf) != 0) return 2;
  return 0;
}
