// The draws and parameters of the DES bridges' prologue on the device ("des_device"): the stage between gdm_des_scan
// and gdm_des_routing / gdm_des_run_batch that "des" and "des_batch" run per sample in Python on the host.  The chain
// and the arithmetic are des_draws.h, the same source gdm_des_draws_host runs, so the two agree bit for bit.
//
// One sample is one dependent chain on one MT19937 stream (init_genrand and the twist are 624-step recurrences, every
// draw depends on the one before): nothing to spread over lanes inside it.  The mapping is one WAVE (a 64-thread
// workgroup) per sample:
//   * all lanes stage the sample's zero_mask words (and the wav route's threshold flags) in LDS;
//   * lane 0 runs the chain on the 624-word state in LDS;
//   * all lanes write the state out and compute the per-node parameters, one node per lane.
// Every output is written with ordinary vector stores; every index is checked in des_draws.h before it forms an address
// and every loop is bounded by the draw budget.
#include "gdm_common.h"
#include "des_draws.h"

#pragma clang fp contract(off)

namespace {

constexpr int kMaxDim = DES_DRAWS_MAX_DIM;

__global__ __launch_bounds__(GDM_WAVE) void des_draws_kernel(
    int route, int B, int S, int dim, const uint32_t* __restrict__ base, const uint64_t* __restrict__ zero_mask,
    const uint8_t* __restrict__ thr_mask, const int32_t* __restrict__ scan_instruments,
    const int32_t* __restrict__ scan_note_levels, const float* __restrict__ params, int n_params,
    const int32_t* __restrict__ instrument_override, uint8_t* __restrict__ src, int32_t* __restrict__ cols,
    int64_t* __restrict__ seed, int64_t* __restrict__ customers, double* __restrict__ loc, double* __restrict__ scale,
    int32_t* __restrict__ queue_cap, int32_t* __restrict__ instruments, int32_t* __restrict__ note_levels,
    uint32_t* __restrict__ mt_key, int32_t* __restrict__ mt_pos, int32_t* __restrict__ has_gauss,
    double* __restrict__ gauss, int32_t* __restrict__ status) {
  __shared__ uint32_t s_key[DES_MT_N];
  __shared__ uint64_t s_zero[kMaxDim];
  __shared__ int32_t s_cols[kMaxDim];
  __shared__ uint8_t s_thr[kMaxDim], s_perm[kMaxDim], s_src[kMaxDim];
  __shared__ int s_status;

  const int b = blockIdx.x, lane = threadIdx.x;
  if (b >= B) return;
  const float* p = params + (int64_t)b * n_params;
  for (int i = lane; i < dim; i += GDM_WAVE) s_zero[i] = zero_mask[(int64_t)b * dim + i];
  if (route == DES_DRAWS_ROUTE_WAV)
    for (int i = lane; i < S; i += GDM_WAVE) s_thr[i] = thr_mask[(int64_t)b * S + i];
  __syncthreads();
  if (lane == 0) {
    int64_t n_customers = 1000, sd = 0;
    int32_t pos = DES_MT_N;
    const int pre = route == DES_DRAWS_ROUTE_MIDI ? des::midi_customers(p[6], &n_customers) : DES_DRAWS_OK;
    const int st = des::draw_chain(route, dim, S, base[b], pre, s_zero, route == DES_DRAWS_ROUTE_WAV ? s_thr : nullptr,
                                   s_key, &pos, s_perm, s_src, s_cols, &sd);
    s_status = st;
    seed[b] = sd;
    customers[b] = n_customers;
    mt_pos[b] = pos;
    has_gauss[b] = 0;
    gauss[b] = 0.0;
    status[b] = st;
  }
  __syncthreads();
  const int st = s_status;
  for (int i = lane; i < DES_MT_N; i += GDM_WAVE) mt_key[(int64_t)b * DES_MT_N + i] = s_key[i];
  const int32_t over = instrument_override ? instrument_override[b] : DES_DRAWS_NO_INSTRUMENT;
  for (int i = lane; i < dim; i += GDM_WAVE) {
    const int64_t o = (int64_t)b * dim + i;
    double l, s;
    int32_t q, ins, note;
    des::node_outputs(route, i, dim, p, s_src[i] != 0, st, scan_instruments[o], scan_note_levels[o], over, &l, &s, &q,
                      &ins, &note);
    src[o] = s_src[i];
    cols[o] = s_cols[i];
    loc[o] = l;
    scale[o] = s;
    queue_cap[o] = q;
    instruments[o] = ins;
    note_levels[o] = note;
  }
}

int check_args(const char* who, int route, int B, int S, int dim, const void* base, const void* zero_mask,
               const void* thr_mask, const void* scan_instruments, const void* scan_note_levels, const void* params,
               int n_params, bool outputs) {
  GDM_REQUIRE(route == DES_DRAWS_ROUTE_MIDI || route == DES_DRAWS_ROUTE_WAV, "%s: route must be 0 (midi) or 1 (wav)", who);
  GDM_REQUIRE(base && zero_mask && scan_instruments && scan_note_levels && params && outputs, "%s: null pointer", who);
  GDM_REQUIRE(B >= 1 && B <= (1 << 20) && dim >= 1 && dim <= kMaxDim && S >= dim && S <= kMaxDim,
              "%s: B >= 1, 1 <= dim <= S <= %d", who, kMaxDim);
  if (route == DES_DRAWS_ROUTE_MIDI) {
    GDM_REQUIRE(n_params >= 7, "%s: the midi route reads gen2 columns 1..6 (n_params >= 7)", who);
  } else {
    GDM_REQUIRE(thr_mask, "%s: the wav route needs the threshold mask", who);
    GDM_REQUIRE(n_params == 2 * dim, "%s: the wav route reads the scan's (2, dim) rows (n_params == 2 * dim)", who);
    GDM_REQUIRE(S / 8 >= 1 && S / 8 <= dim, "%s: the wav route draws S / 8 sources: 1 <= S / 8 <= dim", who);
  }
  return GDM_OK;
}

}  // namespace

extern "C" int gdm_des_draws(int route, int B, int S, int dim, const uint32_t* base, const uint64_t* zero_mask,
                             const uint8_t* thr_mask_or_null, const int32_t* scan_instruments,
                             const int32_t* scan_note_levels, const float* params, int n_params,
                             const int32_t* instrument_override_or_null, uint8_t* src, int32_t* cols, int64_t* seed,
                             int64_t* customers, double* loc, double* scale, int32_t* queue_cap, int32_t* instruments,
                             int32_t* note_levels, uint32_t* mt_key, int32_t* mt_pos, int32_t* has_gauss,
                             double* cached_gauss, int32_t* status, void* stream) {
  const int rc = check_args("gdm_des_draws", route, B, S, dim, base, zero_mask, thr_mask_or_null, scan_instruments,
                            scan_note_levels, params, n_params,
                            src && cols && seed && customers && loc && scale && queue_cap && instruments &&
                                note_levels && mt_key && mt_pos && has_gauss && cached_gauss && status);
  if (rc != GDM_OK) return rc;
  hipLaunchKernelGGL(des_draws_kernel, dim3(B), dim3(GDM_WAVE), 0, (hipStream_t)stream, route, B, S, dim, base,
                     zero_mask, thr_mask_or_null, scan_instruments, scan_note_levels, params, n_params,
                     instrument_override_or_null, src, cols, seed, customers, loc, scale, queue_cap, instruments,
                     note_levels, mt_key, mt_pos, has_gauss, cached_gauss, status);
  GDM_LAUNCH_OK("gdm_des_draws");
  return GDM_OK;
}

extern "C" int gdm_des_draws_host(int route, int B, int S, int dim, const uint32_t* base, const uint64_t* zero_mask,
                                  const uint8_t* thr_mask_or_null, const int32_t* scan_instruments,
                                  const int32_t* scan_note_levels, const float* params, int n_params,
                                  const int32_t* instrument_override_or_null, uint8_t* src, int32_t* cols,
                                  int64_t* seed, int64_t* customers, double* loc, double* scale, int32_t* queue_cap,
                                  int32_t* instruments, int32_t* note_levels, uint32_t* mt_key, int32_t* mt_pos,
                                  int32_t* has_gauss, double* cached_gauss, int32_t* status) {
  const int rc = check_args("gdm_des_draws_host", route, B, S, dim, base, zero_mask, thr_mask_or_null, scan_instruments,
                            scan_note_levels, params, n_params,
                            src && cols && seed && customers && loc && scale && queue_cap && instruments &&
                                note_levels && mt_key && mt_pos && has_gauss && cached_gauss && status);
  if (rc != GDM_OK) return rc;
  uint8_t perm[kMaxDim];
  for (int b = 0; b < B; ++b) {
    const float* p = params + (int64_t)b * n_params;
    int64_t n_customers = 1000, sd = 0;
    int32_t pos = DES_MT_N;
    const int pre = route == DES_DRAWS_ROUTE_MIDI ? des::midi_customers(p[6], &n_customers) : DES_DRAWS_OK;
    const int st = des::draw_chain(route, dim, S, base[b], pre, zero_mask + (int64_t)b * dim,
                                   route == DES_DRAWS_ROUTE_WAV ? thr_mask_or_null + (int64_t)b * S : nullptr,
                                   mt_key + (int64_t)b * DES_MT_N, &pos, perm, src + (int64_t)b * dim,
                                   cols + (int64_t)b * dim, &sd);
    seed[b] = sd;
    customers[b] = n_customers;
    mt_pos[b] = pos;
    has_gauss[b] = 0;
    cached_gauss[b] = 0.0;
    status[b] = st;
    const int32_t over = instrument_override_or_null ? instrument_override_or_null[b] : DES_DRAWS_NO_INSTRUMENT;
    for (int i = 0; i < dim; ++i) {
      const int64_t o = (int64_t)b * dim + i;
      des::node_outputs(route, i, dim, p, src[o] != 0, st, scan_instruments[o], scan_note_levels[o], over, &loc[o],
                        &scale[o], &queue_cap[o], &instruments[o], &note_levels[o]);
    }
  }
  return GDM_OK;
}
