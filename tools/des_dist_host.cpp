// The distribution policy des::AnyDist of csrc/des_sim.h (normal, exponential and uniform nodes) as a stand-alone host
// program for a sanitizer build: tools/des_stats_host.cpp with a kind per node -- the same exactly sized buffers, the
// same files, int32 kind[dim] between scale and qcap in every case.
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I gan_des_midi_music_gen_amd/csrc tools/des_dist_host.cpp -o des_dist_host
//   ./des_dist_host cases.bin stats.bin
//
// tests/test_des_dist.py writes cases in this form and compares with gdm_des_stats_batch_dist_host(math = 1).
#define DES_HOST_WITH_KIND 1
#include "des_stats_host.cpp"
