// extern "C" entry points of the handle (include/starry_process_amd.h): its lifecycle, the error string, host ->
// device staging (SpStage) and scratch, profiling, settings, host constants and Ylm moments, the kernel tables and the
// collective.  The drivers live next to their kernels: sp_lnlike.hip (likelihood, covariances, design matrix),
// sp_linalg.hip (fp64 linear algebra, SPD inverse), sp_grad.hip (gradient), sp_ylm.hip (surface-map posterior).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <dlfcn.h>
#include <cstring>
#include <new>

#include "sp_internal.h"

static thread_local char g_hip_err[256] = "";

const char *sp_set_hip_error(hipError_t e, const char *what) {
  snprintf(g_hip_err, sizeof(g_hip_err), "%s: %s", what, hipGetErrorString(e));
  return g_hip_err;
}

int sp_ensure_scratch(SpScratch &s, size_t bytes, void **out) {
  if (s.bytes < bytes) {
    SP_HIP(hipDeviceSynchronize());
    if (s.ptr) SP_HIP(hipFree(s.ptr));
    s.ptr = nullptr;
    s.bytes = 0;
    hipError_t e = hipMalloc(&s.ptr, bytes);
    if (e != hipSuccess) {
      sp_set_hip_error(e, "hipMalloc(scratch)");
      return SP_ERR_ALLOC;
    }
    s.bytes = bytes;
  }
  *out = s.ptr;
  return SP_OK;
}

extern "C" {

const char *sp_last_hip_error(void) { return g_hip_err; }

int sp_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int sp_create(int ydeg, int udeg, int device, sp_handle **out) {
  if (!out || ydeg < 1 || ydeg > SP_MAX_YDEG || udeg < 0 || udeg > SP_MAX_UDEG)
    return SP_ERR_INVALID;
  *out = nullptr;
  // device == -1: host-only handle.  It serves the host entry points
  // (sp_rTA1, sp_rTA1L, sp_ydeg ...) and nothing else: every device entry
  // point answers SP_ERR_NO_DEVICE.  There is no CPU compute path.
  const bool host_only = device == -1;
  if (!host_only) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 ||
        device >= ndev)
      return SP_ERR_NO_DEVICE;
    SP_HIP(hipSetDevice(device));
  }
  sp_handle *h = new (std::nothrow) sp_handle();
  if (!h) return SP_ERR_ALLOC;
  h->ydeg = ydeg;
  h->udeg = udeg;
  h->N = (ydeg + 1) * (ydeg + 1);
  h->NWIG = sp_nwig_of(ydeg);
  h->device = device;
  h->cs_ring.resize(4);
  const int N = h->N;
  h->l_of.resize(N);
  h->m_of.resize(N);
  h->mirror.resize(N);
  h->m0.resize(ydeg + 1);
  h->blk.resize(ydeg + 2);
  sp_build_index_tables(ydeg, h->l_of.data(), h->m_of.data(), h->mirror.data(),
                        h->m0.data(), h->blk.data());
  sp_build_flux_constants(ydeg, udeg, h->rT, h->A1, h->U1, h->rta1);
  if (host_only) {
    *out = h;
    return SP_OK;
  }

  const size_t d = sizeof(double);
  SP_HIP(hipMalloc((void **)&h->d_l_of, sizeof(int32_t) * N));
  SP_HIP(hipMalloc((void **)&h->d_m_of, sizeof(int32_t) * N));
  SP_HIP(hipMalloc((void **)&h->d_mirror, sizeof(int32_t) * N));
  SP_HIP(hipMalloc((void **)&h->d_blk, sizeof(int32_t) * (ydeg + 2)));
  SP_HIP(hipMalloc((void **)&h->d_Rx90, d * h->NWIG));
  SP_HIP(hipMalloc((void **)&h->d_wnp, d * h->NWIG));
  SP_HIP(hipMalloc((void **)&h->d_Wnp, d * N * N));
  SP_HIP(hipMalloc((void **)&h->d_mean_ylm, d * N));
  SP_HIP(hipMalloc((void **)&h->d_cov_ylm, d * N * N));
  SP_HIP(hipMalloc((void **)&h->d_ez, d * N));
  SP_HIP(hipMalloc((void **)&h->d_Ez, d * N * N));
  SP_HIP(hipMalloc((void **)&h->d_tmpNN, d * N * N));
  h->scratch_bytes = d * (4 * (size_t)N + 64);
  SP_HIP(hipMalloc((void **)&h->d_scratch, h->scratch_bytes));
  SP_HIP(hipMemcpy(h->d_l_of, h->l_of.data(), sizeof(int32_t) * N, hipMemcpyHostToDevice));
  SP_HIP(hipMemcpy(h->d_m_of, h->m_of.data(), sizeof(int32_t) * N, hipMemcpyHostToDevice));
  SP_HIP(hipMemcpy(h->d_mirror, h->mirror.data(), sizeof(int32_t) * N, hipMemcpyHostToDevice));
  SP_HIP(hipMemcpy(h->d_blk, h->blk.data(), sizeof(int32_t) * (ydeg + 2), hipMemcpyHostToDevice));

  h->tune = sp_tuning_from_env();
  {
    hipDeviceProp_t prop;
    h->ncu = hipGetDeviceProperties(&prop, device) == hipSuccess ? prop.multiProcessorCount : 256;
  }
  // Rx(pi/2): the polar-frame rotation every path uses (flux.py:56,61,62,103)
  const double th = 0.5 * M_PI;
  int rc = sp_Rx(h, &th, 1, h->d_Rx90, nullptr, nullptr);
  if (rc != SP_OK) {
    sp_destroy(h);
    return rc;
  }
  SP_HIP(hipDeviceSynchronize());
  *out = h;
  return SP_OK;
}

void sp_destroy(sp_handle *h) {
  if (!h) return;
  if (h->device < 0) {
    delete h;
    return;
  }
  (void)hipSetDevice(h->device);
  (void)hipDeviceSynchronize();
  void *ptrs[] = {h->d_l_of, h->d_m_of,   h->d_mirror, h->d_blk,   h->d_Rx90,
                  h->d_wnp,  h->d_Wnp,    h->d_mean_ylm, h->d_cov_ylm, h->d_ez,
                  h->d_Ez,   h->d_tmpNN,  h->d_scratch, h->d_xp, h->tab_scratch.ptr, h->d_Rxm90, h->d_lamcs,
                  h->d_size_basis};
  for (hipEvent_t e : h->prof_ev) (void)hipEventDestroy(e);
  for (hipEvent_t e : h->gdone) (void)hipEventDestroy(e);
  for (hipStream_t s2 : h->gstream) (void)hipStreamDestroy(s2);
  if (h->gfork) (void)hipEventDestroy(h->gfork);
  if (h->big.ptr) (void)hipFree(h->big.ptr);
  if (h->pix_A1T.ptr) (void)hipFree(h->pix_A1T.ptr);
  for (auto &c : h->cs_ring) {
    if (c.host) (void)hipHostFree(c.host);
    if (c.dev) (void)hipFree(c.dev);
    if (c.done) (void)hipEventDestroy(c.done);
  }
  for (void *p : ptrs)
    if (p) (void)hipFree(p);
  delete h;
}

int sp_ydeg(const sp_handle *h) { return h ? h->ydeg : SP_ERR_INVALID; }
int sp_udeg(const sp_handle *h) { return h ? h->udeg : SP_ERR_INVALID; }
int sp_nylm(const sp_handle *h) { return h ? h->N : SP_ERR_INVALID; }
int sp_nwig(const sp_handle *h) { return h ? h->NWIG : SP_ERR_INVALID; }

}  // extern "C"

namespace {
int sp_stage_acquire(sp_handle *h, size_t doubles, int *slot) {
  const size_t n = h->cs_ring.size();
  int pick = -1;
  for (size_t k = 0; k < n && pick < 0; ++k) {
    const size_t i = ((size_t)h->cs_next + k) % n;
    sp_handle::CsSlot &c = h->cs_ring[i];
    if (!c.used) {
      pick = (int)i;
    } else {
      const hipError_t q = hipEventQuery(c.done);
      if (q == hipSuccess) pick = (int)i;
      else (void)hipGetLastError();     // (hipErrorNotReady is an answer, not a failure to report later)
    }
  }
  if (pick < 0 && n < SP_STAGE_MAX) {
    h->cs_ring.emplace_back();
    pick = (int)n;
  }
  if (pick < 0) {
    pick = h->cs_next % (int)n;
    SP_HIP(hipEventSynchronize(h->cs_ring[pick].done));
  }
  sp_handle::CsSlot &c = h->cs_ring[pick];
  c.used = false;
  if (c.cap < doubles) {
    if (c.host) SP_HIP(hipHostFree(c.host));
    if (c.dev) SP_HIP(hipFree(c.dev));
    c.host = c.dev = nullptr;
    c.cap = 0;
    const size_t cap = doubles < 512 ? 512 : doubles;
    SP_HIP(hipHostMalloc((void **)&c.host, sizeof(double) * cap, hipHostMallocDefault));
    SP_HIP(hipMalloc((void **)&c.dev, sizeof(double) * cap));
    c.cap = cap;
  }
  if (!c.done) SP_HIP(hipEventCreateWithFlags(&c.done, hipEventDisableTiming));
  h->cs_next = (pick + 1) % (int)h->cs_ring.size();
  *slot = pick;
  return SP_OK;
}
}  // namespace

SpStage::SpStage(sp_handle *h, size_t doubles) : h_(h), n_(doubles) {
  rc = sp_stage_acquire(h, doubles, &slot_);
  if (rc) return;
  sp_handle::CsSlot &c = h->cs_ring[slot_];
  c.used = true;
  host = c.host;
}

const double *SpStage::upload(hipStream_t st) {
  sp_handle::CsSlot &c = h_->cs_ring[slot_];
  const hipError_t e = hipMemcpyAsync(c.dev, c.host, sizeof(double) * n_, hipMemcpyHostToDevice, st);
  if (e != hipSuccess) {
    sp_set_hip_error(e, "hipMemcpyAsync(stage)");
    return nullptr;
  }
  st_ = st;
  sent_ = true;
  return c.dev;
}

SpStage::~SpStage() {
  if (slot_ < 0) return;
  sp_handle::CsSlot &c = h_->cs_ring[slot_];
  if (!sent_) {
    c.used = false;
    return;
  }
  const hipError_t e = hipEventRecord(c.done, st_);
  if (e != hipSuccess) {
    // (the slot's event does not follow the copy, which may still be in flight: drained here instead)
    sp_set_hip_error(e, "hipEventRecord(stage)");
    (void)hipStreamSynchronize(st_);
  }
}

extern "C" {

int sp_stream_synchronize(sp_handle *h, void *stream) {
  if (h && h->device < 0) return SP_ERR_NO_DEVICE;
  if (!h) return SP_ERR_INVALID;
  SP_HIP(hipStreamSynchronize((hipStream_t)stream));
  return SP_OK;
}

int sp_Rx(sp_handle *h, const double *theta_host, int nangles, double *R_dev,
          double *dR_dev, void *stream) {
  if (h && h->device < 0) return SP_ERR_NO_DEVICE;
  if (!h || !theta_host || !R_dev || nangles < 0) return SP_ERR_INVALID;
  if (nangles == 0) return SP_OK;
  hipStream_t st = (hipStream_t)stream;
  // cos/sin on the host with libm, like the reference (wigner.h:153-154), staged through the
  // handle's ring: the slot's previous use is waited for on the host (long finished in
  // practice), nothing is allocated, freed or synchronised once the ring has grown
  SpStage cs(h, 2 * (size_t)nangles);
  if (cs.rc) return cs.rc;
  for (int i = 0; i < nangles; ++i) {
    cs.host[2 * i] = std::cos(theta_host[i]);
    cs.host[2 * i + 1] = std::sin(theta_host[i]);
  }
  const double *dcs = cs.upload(st);
  if (!dcs) return SP_ERR_HIP;
  return sp_launch_Rx(h, dcs, nangles, R_dev, dR_dev, st);
}

int sp_rTA1(sp_handle *h, double *rta1_host) {
  if (!h || !rta1_host) return SP_ERR_INVALID;
  memcpy(rta1_host, h->rta1.data(), sizeof(double) * h->N);
  return SP_OK;
}

int sp_rTA1L(sp_handle *h, const double *u_host, int nsets, double *out) {
  if (!h || !out || nsets < 0 || (h->udeg > 0 && !u_host)) return SP_ERR_INVALID;
  for (int i = 0; i < nsets; ++i)
    sp_host_rTA1L(h, u_host ? u_host + (size_t)i * h->udeg : nullptr,
                  out + (size_t)i * h->N);
  return SP_OK;
}

int sp_rTA1L_rev(sp_handle *h, const double *u_host, const double *bf_host, double *bu_host) {
  if (!h || h->udeg < 1 || !u_host || !bf_host || !bu_host) return SP_ERR_INVALID;
  sp_host_rTA1L_rev(h, u_host, bf_host, bu_host);
  return SP_OK;
}

int sp_set_marginal_constants(sp_handle *h, const double *wnp, const double *Wnp) {
  if (h && h->device < 0) return SP_ERR_NO_DEVICE;
  if (!h || !wnp || !Wnp) return SP_ERR_INVALID;
  SP_HIP(hipSetDevice(h->device));
  SP_HIP(hipMemcpy(h->d_wnp, wnp, sizeof(double) * h->NWIG, hipMemcpyHostToDevice));
  SP_HIP(hipMemcpy(h->d_Wnp, Wnp, sizeof(double) * h->N * h->N, hipMemcpyHostToDevice));
  h->have_marginal = true;
  return SP_OK;
}

int sp_set_ylm_moments(sp_handle *h, const double *mean_ylm, const double *cov_ylm) {
  if (h && h->device < 0) return SP_ERR_NO_DEVICE;
  if (!h || !mean_ylm || !cov_ylm) return SP_ERR_INVALID;
  const int N = h->N;
  SP_HIP(hipSetDevice(h->device));
  SP_HIP(hipMemcpy(h->d_mean_ylm, mean_ylm, sizeof(double) * N, hipMemcpyHostToDevice));
  SP_HIP(hipMemcpy(h->d_cov_ylm, cov_ylm, sizeof(double) * N * N, hipMemcpyHostToDevice));
  hipStream_t st = nullptr;
  // ez = R^T mu, Ez = R^T (Sigma + mu mu^T) R  (flux.py:55-62)
  int rc = sp_launch_polar_moments(h, h->d_mean_ylm, h->d_cov_ylm, st);
  if (rc) return rc;
  SP_HIP(hipStreamSynchronize(st));
  h->have_moments = true;
  return SP_OK;
}

int sp_set_ylm_moments_dev(sp_handle *h, const double *mean_ylm_dev,
                           const double *cov_ylm_dev, void *stream) {
  if (h && h->device < 0) return SP_ERR_NO_DEVICE;
  if (!h || !mean_ylm_dev || !cov_ylm_dev) return SP_ERR_INVALID;
  hipStream_t st = (hipStream_t)stream;
  // one launch: resident copies of mu / Sigma, ez and Ez
  int rc = sp_launch_polar_moments(h, mean_ylm_dev, cov_ylm_dev, st);
  if (rc) return rc;
  h->have_moments = true;
  return SP_OK;
}

int sp_profile_begin(sp_handle *h, int max_launches) {
  return sp_profile_begin_kinds(h, max_launches, 1u << SP_PROF_SYRK);
}

int sp_profile_begin_kinds(sp_handle *h, int max_launches, unsigned kind_mask) {
  if (h && h->device < 0) return SP_ERR_NO_DEVICE;
  if (!h || max_launches < 0) return SP_ERR_INVALID;
  h->prof_mask = kind_mask;
  while (h->prof_ev.size() < 2 * (size_t)max_launches) {
    hipEvent_t e;
    SP_HIP(hipEventCreate(&e));
    h->prof_ev.push_back(e);
  }
  h->prof_kind.assign(h->prof_ev.size() / 2, 0);
  h->prof_fl.assign(h->prof_ev.size() / 2, 0.0);
  h->prof_flp.assign(h->prof_ev.size() / 2, 0.0);
  h->prof_n.assign(h->prof_ev.size() / 2, 0);
  h->prof_used = 0;
  h->prof_on = true;
  return SP_OK;
}

int sp_profile_kind(sp_handle *h, int kind, long *launches, double *total_ms, double *flops) {
  return sp_profile_kind_ex(h, kind, launches, total_ms, flops, nullptr);
}

int sp_profile_kind_ex(sp_handle *h, int kind, long *launches, double *total_ms, double *flops, double *flops_padded) {
  if (h && h->device < 0) return SP_ERR_NO_DEVICE;
  if (!h || kind < 0 || kind >= SP_PROF_NKINDS) return SP_ERR_INVALID;
  h->prof_on = false;
  double ms = 0.0, fl = 0.0, flp = 0.0;
  long n = 0;
  for (size_t i = 0; i + 1 < h->prof_used; i += 2) {
    if (h->prof_kind[i / 2] != kind) continue;
    SP_HIP(hipEventSynchronize(h->prof_ev[i + 1]));
    float dt = 0.f;
    SP_HIP(hipEventElapsedTime(&dt, h->prof_ev[i], h->prof_ev[i + 1]));
    ms += dt;
    fl += h->prof_fl[i / 2];
    flp += h->prof_flp[i / 2];
    n += h->prof_n[i / 2];
  }
  if (launches) *launches = n;
  if (total_ms) *total_ms = ms;
  if (flops) *flops = fl;
  if (flops_padded) *flops_padded = flp;
  return SP_OK;
}

int sp_profile_end(sp_handle *h, long *launches, double *total_ms, double *flops) {
  return sp_profile_kind(h, SP_PROF_SYRK, launches, total_ms, flops);
}

int sp_set_lazy_cov(sp_handle *h, int on) {
  if (h && h->device < 0) return SP_ERR_NO_DEVICE;
  if (!h) return SP_ERR_INVALID;
  h->tune.lazy_cov = on ? 1 : 0;
  return SP_OK;
}

int sp_set_defer_norm(sp_handle *h, int on) {
  if (h && h->device < 0) return SP_ERR_NO_DEVICE;
  if (!h || (on != 0 && on != 1)) return SP_ERR_INVALID;
  h->tune.defer_norm = on;
  return SP_OK;
}

// (debug) look-ahead items of the panel launches on / off (sp_cholesky.hip); results agree to rounding
int sp_debug_set_look_ahead(sp_handle *h, int on) {
  if (!h) return SP_ERR_INVALID;
  h->tune.look_ahead = on ? 1 : 0;
  return SP_OK;
}

// (debug) the panel launches' layout by CU and the reduction in the last launch's tail, on / off: same bits
int sp_debug_set_panel_layout(sp_handle *h, int layout, int fuse_reduce) {
  if (!h) return SP_ERR_INVALID;
  h->tune.panel_layout = layout ? 1 : 0;
  h->tune.fuse_reduce = fuse_reduce ? 1 : 0;
  return SP_OK;
}

int sp_get_polar_moments(sp_handle *h, double *ez, double *Ez) {
  if (h && h->device < 0) return SP_ERR_NO_DEVICE;
  if (!h) return SP_ERR_INVALID;
  if (!h->have_moments) return SP_ERR_STATE;
  SP_HIP(hipSetDevice(h->device));
  if (ez) SP_HIP(hipMemcpy(ez, h->d_ez, sizeof(double) * h->N, hipMemcpyDeviceToHost));
  if (Ez)
    SP_HIP(hipMemcpy(Ez, h->d_Ez, sizeof(double) * h->N * h->N, hipMemcpyDeviceToHost));
  return SP_OK;
}

// the lag grid of the kernel table on the device: uploaded when it changes (sp_kernel_table, sp_kernel_table_samples)
int sp_ensure_lag_grid(sp_handle *h, int covpts, const double *xp_host) {
  const int np = covpts + 4;
  const bool same = h->xp_covpts == covpts && (int)h->xp_host.size() == np &&
                    memcmp(h->xp_host.data(), xp_host, sizeof(double) * np) == 0;
  if (same) return SP_OK;
  // new lag grid: (re)allocate and upload once; later calls with the same
  // grid are fully asynchronous
  SP_HIP(hipSetDevice(h->device));
  SP_HIP(hipDeviceSynchronize());
  if (h->d_xp) SP_HIP(hipFree(h->d_xp));
  h->d_xp = nullptr;
  h->xp_covpts = -1;
  SP_HIP(hipMalloc((void **)&h->d_xp, sizeof(double) * np));
  SP_HIP(hipMemcpy(h->d_xp, xp_host, sizeof(double) * np, hipMemcpyHostToDevice));
  h->xp_host.assign(xp_host, xp_host + np);
  h->xp_covpts = covpts;
  return SP_OK;
}

int sp_kernel_table(sp_handle *h, const double *rta1_dev, int ntab, int covpts,
                    const double *xp_host, double *tab_dev, double *meanvar_dev,
                    void *stream) {
  if (h && h->device < 0) return SP_ERR_NO_DEVICE;
  if (!h || !rta1_dev || !xp_host || !tab_dev || !meanvar_dev || ntab < 0 ||
      covpts < 1)
    return SP_ERR_INVALID;
  if (!h->have_marginal || !h->have_moments) return SP_ERR_STATE;
  if (ntab == 0) return SP_OK;
  int rc = sp_ensure_lag_grid(h, covpts, xp_host);
  if (rc) return rc;
  rc = sp_launch_kernel_table(h, rta1_dev, ntab, covpts, h->d_xp, tab_dev,
                              meanvar_dev, (hipStream_t)stream);
  if (rc == SP_OK) h->tab_ntab = ntab;
  return rc;
}

// The kernel tables of B hyperparameter samples in one call (round 6): polar-frame moments ez [B][N], Ez [B][N][N]
// given (sp_polar_moments_samples), table b ntab + i from sample b's moments and flux operator i.
int sp_kernel_table_samples(sp_handle *h, int B, const double *ez_dev, const double *Ez_dev, const double *rta1_dev,
                            int ntab, int covpts, const double *xp_host, double *tab_dev, double *meanvar_dev,
                            void *stream) {
  if (h && h->device < 0) return SP_ERR_NO_DEVICE;
  if (!h || !ez_dev || !Ez_dev || !rta1_dev || !xp_host || !tab_dev || !meanvar_dev || ntab < 0 || covpts < 1 || B < 0)
    return SP_ERR_INVALID;
  if (!h->have_marginal) return SP_ERR_STATE;
  if (ntab == 0 || B == 0) return SP_OK;
  int rc = sp_ensure_lag_grid(h, covpts, xp_host);
  if (rc) return rc;
  return sp_launch_kernel_table(h, rta1_dev, ntab, covpts, h->d_xp, tab_dev, meanvar_dev, (hipStream_t)stream, B,
                                ez_dev, Ez_dev);
}

// The one collective of the path.  RCCL is resolved in the running
// process: the communicator belongs to the caller, so must the library.
int sp_allgather_lnlike(sp_handle *h, void *nccl_comm, const double *local_dev, int count,
                        double *all_dev, void *stream) {
  if (h && h->device < 0) return SP_ERR_NO_DEVICE;
  if (!h || !nccl_comm || !local_dev || !all_dev || count < 0) return SP_ERR_INVALID;
  if (count == 0) return SP_OK;
  typedef int (*allgather_fn)(const void *, void *, size_t, int, void *, hipStream_t);
  static allgather_fn fn = nullptr;
  if (!fn) fn = reinterpret_cast<allgather_fn>(dlsym(RTLD_DEFAULT, "ncclAllGather"));
  if (!fn) return SP_ERR_COMM;
  const int nccl_float64 = 8;  // ncclFloat64 / ncclDouble
  return fn(local_dev, all_dev, (size_t)count, nccl_float64, nccl_comm, (hipStream_t)stream) == 0
             ? SP_OK
             : SP_ERR_COMM;
}

}  // extern "C"
