// engine.hip — host side of the C ABI (include/mpcr.h): model blobs, engines
// (the device model and its tables are compiled by dev_model.h and uploaded
// here), launches, the plant, the CEM context.
#include <hip/hip_runtime.h>
#include <dlfcn.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdarg>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/mpcr.h"
#include "mpcr_device.h"

// kernels: the fused rollout has its own translation units (rollout.hip, built through
// rollout_narrow.hip and rollout_wide.hip; their launchers declared in rollout.h, the launch
// planning over them in rollout_plan.h); cem.hip:
// the CEM distribution step
#include "rollout.h"
#include "rollout_plan.h"
#include "dev_model.h"
#include "step_table.h"

// horizon segments of dual-arm rollouts (rollout_launch): steps per segment
// (0 = one launch) and candidate groups on their own streams.  Measured
// (round 4 sweep; C4 shard 4096 x 100 / C5 rollout 8192 x 50, ms):
// one launch 50.6 / 48.5; 2 groups x 25 steps 47.8 / 47.4, x 13-10 46.7 /
// 45.8, x 7 46.3 / 45.0, x 5-3 46.4-46.6 / 45.1; 3 groups 47.3-49.5; 4
// groups 65-67 (more streams than the process's 4 hardware queues)
#ifndef MPCR_SEG_STEPS_DEFAULT
#define MPCR_SEG_STEPS_DEFAULT 7
#endif
#ifndef MPCR_SEG_GROUPS_DEFAULT
#define MPCR_SEG_GROUPS_DEFAULT 2
#endif
#define MPCR_SEG_MAXG 4
static int env_int_or(const char* name, int dflt) {
  const char* v = getenv(name);
  return v ? atoi(v) : dflt;
}
#include "cem.hip"

namespace mpcr {
// argmin with NaN-first / first-index semantics over cost[i*stride]
__global__ void __launch_bounds__(256) argmin_kernel(const float* __restrict__ cost, int stride, int n, int base,
                                                     unsigned long long* key) {
  unsigned long long best = ~0ull;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const float c = cost[(size_t)i * stride];
    const uint32_t u = __float_as_uint(c);
    const uint32_t k = isnan(c) ? 0u : ((u & 0x80000000u) ? ~u : (u | 0x80000000u));
    const unsigned long long k64 = ((unsigned long long)k << 32) | (uint32_t)(base + i);
    best = k64 < best ? k64 : best;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long other = __shfl_xor(best, o);
    best = other < best ? other : best;
  }
  if ((threadIdx.x & 63) == 0) atomicMin(key, best);
}

__global__ void fill_u64(unsigned long long* p, unsigned long long v) { p[blockIdx.x] = v; }  // one block per word

}  // namespace mpcr

using namespace mpcr;

struct mpcr_model {
  mpcr_model_t m;
};

// Device allocations with one owner, freed together when it goes: an engine's
// buffers, a plant's, a debug entry's temporaries.  The first failure sticks
// (later calls return null), so a caller makes all its allocations and checks
// rc once: MPCR_ENOMEM for an allocation, MPCR_EHIP for a copy.
struct DevBufs {
  std::vector<void*> list;
  int rc = MPCR_OK;
  DevBufs() = default;
  DevBufs(const DevBufs&) = delete;
  DevBufs& operator=(const DevBufs&) = delete;
  ~DevBufs() {
    for (void* p : list) (void)hipFree(p);
  }
  // n elements; the first nsrc of them uploaded from src
  template <class T>
  T* alloc(size_t n, const T* src = nullptr, size_t nsrc = 0) {
    void* p = nullptr;
    if (rc) return nullptr;
    if (hipMalloc(&p, sizeof(T) * n) != hipSuccess) { rc = MPCR_ENOMEM; return nullptr; }
    list.push_back(p);
    if (nsrc && hipMemcpy(p, src, sizeof(T) * nsrc, hipMemcpyHostToDevice) != hipSuccess) rc = MPCR_EHIP;
    return static_cast<T*>(p);
  }
  template <class T>
  T* upload(const std::vector<T>& v) { return alloc<T>(v.size() ? v.size() : 1, v.data(), v.size()); }
};

struct mpcr_engine {
  int device = 0, max_n = 0, H = 0, nbasis = 0;
  mpcr_model_t host;
  DevModel dev;
  DevBufs mem;  // every device buffer of the engine: the named ones below and the model's tables
  DevModel* d_model = nullptr;
  float* d_pdot = nullptr;
  // staging (host-pointer calls)
  float* d_in = nullptr;
  float* d_cost = nullptr;
  float* d_theta = nullptr;
  float* d_thetadot = nullptr;
  unsigned long long* d_key = nullptr;
  int* d_status = nullptr;
  int* d_idx = nullptr;
  float* d_slot_prev = nullptr;  // max_n x nslot: cost_c history of the pairs not held in registers
  float* d_jx = nullptr;         // max_n x (MAXEFC - JL) x LDJ: J rows past the LDS ones
  float* d_td = nullptr;         // (max_n + 1) x nctrl x H joint-velocity table (thetadot not requested)
  short* d_hints = nullptr;      // max_n x NHINT x 2 (dual-arm class): hull-climb starts
  unsigned* d_pace = nullptr;    // MPCR_PACE_SLOTS: the rollout kernel's per-wave-slot progress (pacing)
  float* d_mslab = nullptr;      // (max_n + 1) x NVW x LD: the dual-arm class's mass matrices
  // horizon segments of the dual-arm class (rollout_launch): steps per
  // segment, candidate groups and their streams / fork-join events
  float* d_seg = nullptr;        // max_n x SEG_STRIDE
  int seg_steps = 0, seg_groups = 1, seg_min_n = 0;
  hipStream_t seg_stream[MPCR_SEG_MAXG] = {};
  hipEvent_t seg_event[MPCR_SEG_MAXG + 1] = {};
  bool wide = false;  // kernel variant: rollout_kernel<32, 32, 72, true>
};

// The step table (step_table.h) and the device model (dev_model.h) are built
// from the same model_frames() and the same row-value functions
// (model_frames.h); their constants are the kernel's.
static_assert(ST_NB == DX_NB && ST_NV == DX_NV && ST_NP == DX_NP && ST_NJ == DX_NJ && ST_NEQ == DX_NEQ,
              "step table capacities = device model capacities");
static_assert(ST_BK_FREE == BK_FREE && ST_BK_HINGE == BK_HINGE && ST_BK_SLIDE == BK_SLIDE && ST_BK_WELD == BK_WELD,
              "body kinds");
static_assert(ST_MINVAL == kMinVal && ST_MINIMP == kMinImp && ST_MAXIMP == kMaxImp, "the kernel's impedance constants");
static thread_local std::string g_err;

static int fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
static int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

#define HIPCHK(x)                                                                         \
  do {                                                                                    \
    hipError_t e_ = (x);                                                                  \
    if (e_ != hipSuccess) return fail(MPCR_EHIP, "%s: %s", #x, hipGetErrorString(e_));  \
  } while (0)

extern "C" const char* mpcr_last_error(void) { return g_err.c_str(); }
extern "C" int mpcr_abi_version(void) { return MPCR_ABI_VERSION; }

extern "C" int mpcr_device_arch(int device, char* buf, int buflen) {
  hipDeviceProp_t prop;
  HIPCHK(hipGetDeviceProperties(&prop, device));
  snprintf(buf, buflen, "%s", prop.gcnArchName);
  return MPCR_OK;
}

// ---------------------------------------------------------------------------
// models

static int check_model(const mpcr_model_t& m) {
  if (m.magic != MPCR_MODEL_MAGIC) return fail(MPCR_EMODEL, "bad model magic 0x%x", m.magic);
  if (m.version != MPCR_MODEL_VERSION) return fail(MPCR_EMODEL, "model version %u != %d", m.version, MPCR_MODEL_VERSION);
  if (m.nbytes != sizeof(mpcr_model_t)) return fail(MPCR_EMODEL, "model size %u != %zu", m.nbytes, sizeof(mpcr_model_t));
  if (m.nbody > MPCR_MAX_BODY || m.njnt > MPCR_MAX_JNT || m.nv > MPCR_MAX_DOF || m.nq > MPCR_MAX_NQ ||
      m.ngeom > MPCR_MAX_GEOM || m.npair > MPCR_MAX_PAIR || m.neq > MPCR_MAX_EQ || m.nctrl > MPCR_MAX_CTRL ||
      m.nu > MPCR_MAX_ACT || m.nhullv > MPCR_MAX_HULLV || m.nhulla > MPCR_MAX_HULLA || m.nu < 0 || m.nhullv < 0 ||
      m.nhulla < 0)
    return fail(MPCR_EMODEL, "model exceeds blob capacity");
  if ((m.integrator != MPCR_INT_EULER && m.integrator != MPCR_INT_IMPLICITFAST) || (m.cone != MPCR_CONE_PYRAMIDAL && m.cone != MPCR_CONE_ELLIPTIC))
    return fail(MPCR_EMODEL, "only Euler / implicitfast with pyramidal or elliptic cones supported");
  if (m.nten < 0 || m.nten > MPCR_MAX_TEN) return fail(MPCR_EMODEL, "model exceeds blob capacity");
  if (m.density != 0) return fail(MPCR_EMODEL, "fluid density (inertia-box drag terms) not supported");
  if (m.viscosity != 0 && m.integrator != MPCR_INT_EULER)
    return fail(MPCR_EMODEL, "fluid viscosity with implicit integration not supported");
  for (int g = 0; g < m.ngeom; g++) {
    if (m.geom_hulladr[g] >= 0 && m.geom_hulladr[g] + m.geom_hullnum[g] > m.nhullv)
      return fail(MPCR_EMODEL, "geom %d hull outside the vertex table", g);
  }
  for (int v = 0; v < m.nhullv; v++)
    if (m.hull_adjadr[v] < 0 || m.hull_adjadr[v] + m.hull_adjnum[v] > m.nhulla)
      return fail(MPCR_EMODEL, "hull vertex %d adjacency outside the table", v);
  for (int k = 0; k < m.nhulla; k++)
    if (m.hull_adj[k] < 0 || m.hull_adj[k] >= m.nhullv) return fail(MPCR_EMODEL, "bad hull adjacency entry");
  for (int p = 0; p < m.npair; p++)
    for (int g : {m.pair_geom1[p], m.pair_geom2[p]})
      if (m.geom_type[g] == MPCR_GEOM_MESH && m.geom_hulladr[g] < 0)
        return fail(MPCR_EMODEL, "mesh geom %d in a pair has no convex hull", g);
  // polygon faces (v7): every index the manifold follows stays in its table
  if (m.nface < 0 || m.nface > MPCR_MAX_FACE || m.nfacev < 0 || m.nfacev > MPCR_MAX_FACEV || m.nvface < 0 ||
      m.nvface > MPCR_MAX_VFACE)
    return fail(MPCR_EMODEL, "model faces exceed blob capacity");
  for (int g = 0; g < m.ngeom; g++) {
    if (m.geom_faceadr[g] >= 0 && m.geom_faceadr[g] + m.geom_facenum[g] > m.nface)
      return fail(MPCR_EMODEL, "geom %d faces outside the face table", g);
    if (m.geom_cornadr[g] >= 0 && (m.geom_type[g] != MPCR_GEOM_BOX || m.geom_cornadr[g] + 8 > m.nhullv))
      return fail(MPCR_EMODEL, "geom %d box corners outside the vertex table", g);
    if (m.geom_faceadr[g] >= 0 && m.geom_type[g] == MPCR_GEOM_BOX && m.geom_cornadr[g] < 0)
      return fail(MPCR_EMODEL, "box geom %d has faces but no corners", g);
  }
  for (int f = 0; f < m.nface; f++)
    if (m.face_vadr[f] < 0 || m.face_vnum[f] < 3 || m.face_vnum[f] > MPCR_FACE_MAXV ||
        m.face_vadr[f] + m.face_vnum[f] > m.nfacev)
      return fail(MPCR_EMODEL, "face %d polygon outside the face-vertex table", f);
  for (int k = 0; k < m.nfacev; k++)
    if (m.face_vert[k] < 0 || m.face_vert[k] >= m.nhullv) return fail(MPCR_EMODEL, "bad face vertex entry");
  if (m.nface > 0)
    for (int v = 0; v < m.nhullv; v++)
      if (m.vert_faceadr[v] < 0 || m.vert_faceadr[v] + m.vert_facenum[v] > m.nvface)
        return fail(MPCR_EMODEL, "hull vertex %d face list outside the table", v);
  for (int k = 0; k < m.nvface; k++)
    if (m.vert_face[k] < 0 || m.vert_face[k] >= m.nface) return fail(MPCR_EMODEL, "bad vertex face entry");
  for (int p = 0; p < m.npair; p++)  // a polyhedron pair's geoms carry faces
    if (m.pair_func[p] == MPCR_COL_CONVEX && m.pair_ncon[p] == 4)
      for (int g : {m.pair_geom1[p], m.pair_geom2[p]})
        if (m.geom_faceadr[g] < 0) return fail(MPCR_EMODEL, "polyhedron-pair geom %d has no faces", g);
  return MPCR_OK;
}

extern "C" int mpcr_model_from_blob(const void* blob, size_t nbytes, mpcr_model** out) {
  if (!blob || !out) return fail(MPCR_EINVAL, "null argument");
  if (nbytes != sizeof(mpcr_model_t)) return fail(MPCR_EMODEL, "blob size %zu != %zu", nbytes, sizeof(mpcr_model_t));
  auto* h = new mpcr_model;
  std::memcpy(&h->m, blob, sizeof(mpcr_model_t));
  int rc = check_model(h->m);
  if (rc) { delete h; return rc; }
  *out = h;
  return MPCR_OK;
}

// MJCF: the compiler in libmpcr_mjcf.so (next to this library), dlopened on
// first use so the engine itself never links Python
static int load_mjcf(const char* path, double timestep, mpcr_model** out) {
  using compile_fn = int (*)(const char*, double, void**, size_t*, char*, int);
  using free_fn = void (*)(void*);
  static void* so = nullptr;
  if (!so) {
    Dl_info info;
    std::string dir = ".";
    if (dladdr(reinterpret_cast<void*>(&mpcr_model_load), &info) && info.dli_fname) {
      dir = info.dli_fname;
      size_t k = dir.find_last_of('/');
      dir = k == std::string::npos ? std::string(".") : dir.substr(0, k);
    }
    so = dlopen((dir + "/libmpcr_mjcf.so").c_str(), RTLD_NOW | RTLD_LOCAL);
    if (!so) return fail(MPCR_EMODEL, "MJCF compiler unavailable: %s", dlerror());
  }
  auto compile = reinterpret_cast<compile_fn>(dlsym(so, "mpcr_mjcf_compile"));
  auto release = reinterpret_cast<free_fn>(dlsym(so, "mpcr_mjcf_free"));
  if (!compile || !release) return fail(MPCR_EMODEL, "libmpcr_mjcf.so lacks its entry points");
  void* blob = nullptr;
  size_t n = 0;
  char err[512] = {0};
  if (compile(path, timestep, &blob, &n, err, sizeof(err)) != 0) return fail(MPCR_EMODEL, "MJCF %s: %s", path, err);
  int rc = mpcr_model_from_blob(blob, n, out);
  release(blob);
  return rc;
}

static bool is_mjcf(const char* path) {
  const size_t n = std::strlen(path);
  if (n >= 4 && std::strcmp(path + n - 4, ".xml") == 0) return true;
  FILE* f = fopen(path, "rb");
  if (!f) return false;
  int c;
  while ((c = fgetc(f)) == ' ' || c == '\n' || c == '\r' || c == '\t') {
  }
  fclose(f);
  return c == '<';
}

extern "C" int mpcr_model_load(const char* path, double timestep, mpcr_model** out) {
  if (!path || !out) return fail(MPCR_EINVAL, "null argument");
  if (is_mjcf(path)) return load_mjcf(path, timestep, out);
  FILE* f = fopen(path, "rb");
  if (!f) return fail(MPCR_EINVAL, "cannot open %s", path);
  std::vector<char> buf(sizeof(mpcr_model_t) + 1);
  size_t n = fread(buf.data(), 1, buf.size(), f);
  fclose(f);
  int rc = mpcr_model_from_blob(buf.data(), n, out);
  if (rc) return rc;
  if (timestep > 0) (*out)->m.timestep = timestep;
  return MPCR_OK;
}

extern "C" int mpcr_model_set_timestep(mpcr_model* m, double timestep) {
  if (!m || !(timestep > 0)) return fail(MPCR_EINVAL, "bad timestep");
  m->m.timestep = timestep;
  return MPCR_OK;
}

extern "C" int mpcr_model_info(const mpcr_model* m, int* nq, int* nv, int* nslot, int* nctrl, int* npair) {
  if (!m) return fail(MPCR_EINVAL, "null model");
  if (nq) *nq = m->m.nq;
  if (nv) *nv = m->m.nv;
  if (nslot) *nslot = m->m.nslot;
  if (nctrl) *nctrl = m->m.nctrl;
  if (npair) *npair = m->m.npair;
  return MPCR_OK;
}

extern "C" int mpcr_model_actuators(const mpcr_model* m, int* nu, double* ctrlrange, int* limited) {
  if (!m) return fail(MPCR_EINVAL, "null model");
  if (nu) *nu = m->m.nu;
  for (int a = 0; a < m->m.nu; a++) {
    if (ctrlrange) { ctrlrange[2 * a] = m->m.act_ctrlrange[a][0]; ctrlrange[2 * a + 1] = m->m.act_ctrlrange[a][1]; }
    if (limited) limited[a] = m->m.act_ctrllimited[a] != 0;
  }
  return MPCR_OK;
}

extern "C" int mpcr_model_geom_poses(const mpcr_model* m, int* ngeom, float* block, int* model_geom_id,
                                     int* is_static) {
  if (!m) return fail(MPCR_EINVAL, "null model");
  const int ng = model_geom_poses(m->m, block, model_geom_id, is_static);
  if (ng < 0) return fail(MPCR_EMODEL, "model exceeds blob capacity");
  if (ngeom) *ngeom = ng;
  return MPCR_OK;
}

extern "C" int mpcr_model_slots(const mpcr_model* m, int* nslot, int* geom1, int* geom2, int* pair) {
  if (!m) return fail(MPCR_EINVAL, "null model");
  const int ns = model_slots(m->m, geom1, geom2, pair);
  if (ns < 0) return fail(MPCR_EMODEL, "model exceeds blob capacity");
  if (nslot) *nslot = ns;
  return MPCR_OK;
}

extern "C" void mpcr_model_free(mpcr_model* m) { delete m; }

// the support start table's scramble seed (dev_model.h hull_start_table; the
// start-independence tests), read at engine creation
static std::atomic<uint64_t> g_start_scramble{0};

extern "C" int64_t mpcr_model_hull_starts(const mpcr_model* m, int R, int32_t* geom_adr, int32_t* cells,
                                          uint8_t* exact, int64_t cap) {
  if (!m) return fail(MPCR_EINVAL, "null model");
  if (R == 0) R = MPCR_LUT_R;
  if (R < 1 || R > 1024) return fail(MPCR_EINVAL, "table resolution %d outside 1..1024", R);
  std::vector<int32_t> adr(std::max(1, m->m.ngeom));
  const int64_t n = hull_start_table(m->m, R, 0, adr.data(), nullptr);
  if (geom_adr) std::copy(adr.begin(), adr.begin() + m->m.ngeom, geom_adr);
  if ((cells || exact) && cap >= n) {
    std::vector<int32_t> own;
    if (!cells) own.resize(n), cells = own.data();
    hull_start_table(m->m, R, 0, nullptr, cells);
    if (exact) hull_exact_cells(m->m, R, adr.data(), cells, exact);
  }
  return n;
}

extern "C" uint64_t mpcr_set_hull_start_scramble(uint64_t seed) { return g_start_scramble.exchange(seed); }

// ---------------------------------------------------------------------------
// engines

extern "C" int mpcr_engine_create(const mpcr_model* m, int device, int max_n, int horizon, const float* pdot,
                                  int nbasis, mpcr_engine** out) {
  if (!m || !out || max_n <= 0 || horizon <= 0 || !pdot || nbasis <= 0 || nbasis > 12)
    return fail(MPCR_EINVAL, "bad engine arguments");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(MPCR_ENODEV, "no HIP device");
  if (device < 0 || device >= ndev) return fail(MPCR_ENODEV, "device %d out of range (%d)", device, ndev);
  HIPCHK(hipSetDevice(device));
  hipDeviceProp_t prop;
  HIPCHK(hipGetDeviceProperties(&prop, device));
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail(MPCR_ENODEV, "device %d is %s; libmpcr is built for gfx950 only", device, prop.gcnArchName);
  auto* e = new mpcr_engine;
  auto refuse = [e](int rc) { mpcr_engine_free(e); return rc; };
  e->device = device;
  e->max_n = max_n;
  e->H = horizon;
  e->nbasis = nbasis;
  e->host = m->m;
  // compile (dev_model.h): the device model and the host images of its tables
  const mpcr_model_t& h = e->host;
  DevOptions opt;
  opt.newton_reuse = env_int_or("MPCR_NEWTON_REUSE", 1);
  opt.narrow_eager = env_int_or("MPCR_NARROW_EAGER", 0);
  opt.lane_work = env_int_or("MPCR_LANE_WORK", 1);
  opt.m_slab = env_int_or("MPCR_M_SLAB", 0);
  opt.w2_lead_max = env_int_or("MPCR_W2_LEAD_MAX", W2_LEAD_MAX);
  opt.start_scramble = g_start_scramble.load();
  DevTables t;
  std::string err;
  if (int rc = compile_dev_model(h, opt, e->dev, t, err)) return refuse(fail(rc, "%s", err.c_str()));
  e->wide = needs_wide(h, e->dev);
  std::vector<StepTable> step;
  std::vector<StepRecords> recs;
  if (!e->wide) {
    // built once: the model and the timestep are fixed for the engine's life
    // (single-arm kernels only: the dual-arm ones never read it)
    step.resize(1);
    recs.resize(1);
    if (build_step_table(h, step[0]) != 0 || build_step_records(h, recs[0]) != 0)
      return refuse(fail(MPCR_EMODEL, "model exceeds the step table's capacities"));
  }
  // upload: the tables the device model points to (hulls, start table, faces,
  // cone cells), the model with the narrow kernels' step table directly behind
  // it (step_table.h: the kernels address it as model + 1) and the load
  // records behind that, then the staging
  // and scratch buffers
  DevBufs& mem = e->mem;
  if (h.nhullv > 0) {
    e->dev.hull_vert = as_gmem(mem.upload(t.hull_vert));
    e->dev.hull_info = as_gmem(mem.upload(t.hull_info));
    e->dev.hull_adjv = as_gmem(mem.upload(t.hull_adjv));
    e->dev.hull_head = as_gmem(mem.upload(t.hull_head));
    e->dev.hull_lut = as_gmem(mem.upload(t.hull_lut));
  }
  if (h.nface > 0) {
    e->dev.face_plane = as_gmem(mem.upload(t.face_plane));
    e->dev.face_vinfo = as_gmem(mem.upload(t.face_vinfo));
    e->dev.face_vert = as_gmem(mem.alloc<int>(h.nfacev, h.face_vert, h.nfacev));
    e->dev.vert_finfo = as_gmem(mem.upload(t.vert_finfo));
    e->dev.vert_face = as_gmem(mem.alloc<int>(h.nvface, h.vert_face, h.nvface));
    e->dev.cone_cell = as_gmem(mem.upload(t.cone_cell));
    e->dev.cone_face = as_gmem(mem.upload(t.cone_face));
  }
  static_assert(sizeof(DevModel) % alignof(mpcr::StepTable) == 0, "the step table's alignment behind the device model");
  const int nc = h.nctrl;
  const size_t rows = (size_t)max_n + 1;  // per-candidate scratch slabs: one spare row of slack
  const size_t nhints = 2 * (size_t)max_n * (e->wide ? SmemW::NHINT : 1);
  static_assert(sizeof(StepTable) % alignof(mpcr::StepRecords) == 0, "the load records' alignment behind the step table");
  e->d_model = reinterpret_cast<DevModel*>(mem.alloc<char>(sizeof(DevModel) + sizeof(StepTable) + sizeof(StepRecords),
                                                           reinterpret_cast<const char*>(&e->dev), sizeof(DevModel)));
  if (e->d_model && !e->wide &&
      (hipMemcpy(e->d_model + 1, step.data(), sizeof(StepTable), hipMemcpyHostToDevice) != hipSuccess ||
       hipMemcpy(reinterpret_cast<char*>(e->d_model + 1) + sizeof(StepTable), recs.data(), sizeof(StepRecords),
                 hipMemcpyHostToDevice) != hipSuccess))
    mem.rc = MPCR_EHIP;
  e->d_pdot = mem.alloc<float>((size_t)horizon * nbasis, pdot, (size_t)horizon * nbasis);
  e->d_in = mem.alloc<float>((size_t)max_n * nc * (horizon > nbasis ? horizon : nbasis));
  e->d_cost = mem.alloc<float>((size_t)max_n * 4);
  e->d_theta = mem.alloc<float>((size_t)max_n * nc * horizon);
  e->d_thetadot = mem.alloc<float>((size_t)max_n * nc * horizon);
  e->d_key = mem.alloc<unsigned long long>(1);
  e->d_status = mem.alloc<int>(max_n);
  e->d_idx = mem.alloc<int>(max_n);
  e->d_slot_prev = mem.alloc<float>(rows * (h.nslot > 0 ? h.nslot : 1));
  e->d_jx = mem.alloc<float>(rows * (e->wide ? (SmemW::MAXEFC - SmemW::JL + 1) * SmemW::LDJ
                                             : (SmemN::MAXEFC - SmemN::JL + 1) * SmemN::LDJ));
  e->d_hints = mem.alloc<short>(nhints);
  e->d_pace = mem.alloc<unsigned>(MPCR_PACE_SLOTS);
  e->d_mslab = mem.alloc<float>(rows * (e->wide ? SmemW::NVW * SmemW::LD : 1));
  e->d_td = mem.alloc<float>(rows * (size_t)(nc > 0 ? nc : 1) * (size_t)horizon);
  if (!mem.rc && (hipMemset(e->d_hints, 0xff, sizeof(short) * nhints) != hipSuccess ||
                  hipMemset(e->d_pace, 0xff, sizeof(unsigned) * MPCR_PACE_SLOTS) != hipSuccess))
    mem.rc = MPCR_EHIP;
  if (e->wide) {
    // horizon segments (MPCR_SEG_STEPS / MPCR_SEG_GROUPS override the defaults)
    e->seg_steps = env_int_or("MPCR_SEG_STEPS", MPCR_SEG_STEPS_DEFAULT);
    e->seg_groups = std::max(1, std::min(MPCR_SEG_MAXG, env_int_or("MPCR_SEG_GROUPS", MPCR_SEG_GROUPS_DEFAULT)));
    if (e->seg_steps > 0 && e->seg_steps < horizon) {
      // a batch the device holds in one round gains nothing: its blocks all
      // start together (the one-wave variant's resident blocks per CU x CUs)
      int occ[6] = {0, 0, 0, 0, 0, 0}, ncu = 0;
      if (rollout_occupancy(occ) == hipSuccess &&
          hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess)
        e->seg_min_n = occ[3] * ncu;
      e->d_seg = mem.alloc<float>((size_t)max_n * SEG_STRIDE);
      bool ok = e->d_seg != nullptr;
      for (int g = 0; ok && e->seg_groups > 1 && g < e->seg_groups; g++)
        ok = hipStreamCreateWithFlags(&e->seg_stream[g], hipStreamNonBlocking) == hipSuccess;
      for (int g = 0; ok && e->seg_groups > 1 && g <= e->seg_groups; g++)
        ok = hipEventCreateWithFlags(&e->seg_event[g], hipEventDisableTiming) == hipSuccess;
      if (!ok && !mem.rc) mem.rc = MPCR_ENOMEM;
    }
  }
  if (mem.rc)
    return refuse(fail(mem.rc, "%s", mem.rc == MPCR_ENOMEM ? "device allocation failed" : "upload to the device failed"));
  *out = e;
  return MPCR_OK;
}

extern "C" void mpcr_engine_free(mpcr_engine* e) {
  if (!e) return;
  for (int g = 0; g < MPCR_SEG_MAXG; g++)
    if (e->seg_stream[g]) (void)hipStreamDestroy(e->seg_stream[g]);
  for (int g = 0; g <= MPCR_SEG_MAXG; g++)
    if (e->seg_event[g]) (void)hipEventDestroy(e->seg_event[g]);
  delete e;  // its DevBufs frees the device buffers
}

// per-call parameter block of the kernel (RolloutArgs::par layout)
static void fill_par(float* par, int nc, const double* q0, const float* w, const float* ptgt, const float* qtgt) {
  for (int k = 0; k < PAR_N; k++) par[k] = 0.f;
  if (q0)
    for (int k = 0; k < nc; k++) par[PAR_Q0 + k] = (float)q0[k];
  for (int k = 0; k < 3; k++) { par[PAR_W + k] = w[k]; par[PAR_PT + k] = ptgt[k]; }
  for (int k = 0; k < 4; k++) par[PAR_QT + k] = qtgt[k];
}

struct Launch {
  const float* in = nullptr;
  int layout = 0, n = 0, index_base = 0, plant = 0;
  const float* dpar = nullptr;  // device parameter block (else par)
  float par[PAR_N] = {};
  float* state = nullptr;
  float *cost4 = nullptr, *theta = nullptr, *thetadot = nullptr, *trace_eef = nullptr, *trace_slots = nullptr;
  unsigned long long* key = nullptr;
  int* status = nullptr;
  float* dbg = nullptr;
  bool reset_key = false;
  int nprob = 1, prob_n = 0;  // nprob > 1: problems of prob_n candidates each (0: one problem)
  // the call's blocks (rollout.h: start / final_state, ctrl, geom_pose, strides in floats; the scenarios per
  // planning problem that share its input rows, 0: none; the target schedule, null: the parameter block's target)
  CallBlocks blk = {};
  SlotWArgs sw = {};  // the contact slots' weights (rollout.h; null: every slot at 1)
  StepWArgs stw = {};  // the cost weights per step (rollout.h; null: every step at 1)
};

// the kernel's arguments for launch l of engine e (the one place they are filled)
static int rollout_args(const mpcr_engine* e, const Launch& l, RolloutArgs& a) {
  std::memset(&a, 0, sizeof(a));
  a.m = e->d_model;
  a.input = l.in;
  a.pdot = e->d_pdot;
  a.cost4 = l.cost4;
  a.theta = l.theta;
  a.thetadot = l.thetadot;
  a.best_key = l.key;
  a.status = l.status;
  a.trace_eef = l.trace_eef;
  a.trace_slots = l.trace_slots;
  a.slot_prev = e->d_slot_prev;
  a.jx = e->d_jx;
  a.tdscratch = e->d_td;
  a.hints = e->d_hints;
  a.pace = e->d_pace;
  a.mslab = e->d_mslab;
  a.dpar = l.dpar;
  a.state = l.state;
  a.plant = l.plant;
  a.dbg = l.dbg;
  a.layout = l.layout;
  a.n = l.n;
  a.H = e->H;
  a.nbasis = e->nbasis;
  a.index_base = l.index_base;
  a.nctrl = e->host.nctrl;
  a.nslot = e->host.nslot;
  a.seg_state = e->d_seg;
  a.seg = e->d_seg ? e->seg_steps : 0;
  a.seg_min_n = e->seg_min_n;
  a.prob_n = l.prob_n;
  a.prob_off = 0;
  // a call with a device parameter block carries its CallBlocks in par's
  // bytes (rollout.h; null pointers when it has no blocks) and never
  // parameter values, so has_state() cannot read those as pointers
  if (l.dpar) {
    a.blk = l.blk;
    a.sw = l.sw;
  } else {
    const StateArgs& s = l.blk.st;
    if (s.start || s.final_state || s.ctrl || s.geom_pose || l.blk.nscen || l.blk.tg.target || l.sw.slot_w ||
        l.stw.step_w)
      return fail(MPCR_EINVAL, "state, control, geom-pose, slot-weight and step-weight blocks need a device "
                               "parameter block");
    std::memcpy(a.par, l.par, sizeof(a.par));
  }
  return MPCR_OK;
}

static int launch_rollout(mpcr_engine* e, const Launch& l, hipStream_t st) {
  RolloutArgs a;
  if (int rc = rollout_args(e, l, a)) return rc;
  if (l.key && l.reset_key) hipLaunchKernelGGL(fill_u64, dim3(l.nprob), dim3(1), 0, st, l.key, ~0ull);
  // (the step weights ride beside the arguments, as the kernels' third: rollout.h StepWArgs)
  rollout_launch(e->wide, a, (const DevModel*)e->d_model, l.n, st, e->seg_groups, e->seg_stream,
                 e->seg_event, l.stw);
  HIPCHK(hipGetLastError());
  return MPCR_OK;
}

extern "C" int mpcr_set_two_wave_max_n(int n) { return rollout_set_wpc2_max_n(n); }

extern "C" int mpcr_engine_dispatches(const mpcr_engine* e, int n, int* out) {
  if (!e || !out) return fail(MPCR_EINVAL, "null argument");
  if (n < 0 || n > e->max_n) return fail(MPCR_EINVAL, "n=%d outside [0, max_n=%d]", n, e->max_n);
  RolloutArgs a;
  Launch l;
  l.n = n;
  if (int rc = rollout_args(e, l, a)) return rc;
  *out = rollout_dispatches(e->wide, a, n, e->seg_groups, e->seg_stream[0] != nullptr, plan_thresholds());
  return MPCR_OK;
}

extern "C" int mpcr_rollout_occupancy(int device, int* info) {
  if (!info) return fail(MPCR_EINVAL, "null argument");
  HIPCHK(hipSetDevice(device));
  HIPCHK(rollout_occupancy(info));
  return MPCR_OK;
}

extern "C" int mpcr_selftest_reduce(int device, const float* in, int nvec, float* out) {
  if (!in || !out || nvec < 1 || nvec > 65536) return fail(MPCR_EINVAL, "selftest_reduce: null argument or nvec outside 1..65536");
  HIPCHK(hipSetDevice(device));
  HIPCHK(rollout_selftest_reduce(in, nvec, out));
  return MPCR_OK;
}

static int check_layout(int layout) {
  if (layout != MPCR_LAYOUT_XI && layout != MPCR_LAYOUT_THETADOT) return fail(MPCR_EINVAL, "bad layout %d", layout);
  return MPCR_OK;
}

// a host-pointer entry's input, n rows of the layout, into the engine's staging buffer
static int stage_input(mpcr_engine* e, const float* input, int layout, int n, hipStream_t st) {
  const size_t cols = (size_t)e->host.nctrl * (layout == MPCR_LAYOUT_XI ? e->nbasis : e->H);
  HIPCHK(hipMemcpyAsync(e->d_in, input, sizeof(float) * n * cols, hipMemcpyHostToDevice, st));
  return MPCR_OK;
}

extern "C" int mpcr_rollout_cost(mpcr_engine* e, const float* input, int layout, int n, const double* q0,
                                 const float* w, const float* ptgt, const float* qtgt, float* cost4, float* theta,
                                 float* thetadot, uint64_t* best_key, int index_base, int* status, int flags,
                                 void* stream) {
  if (!e || !q0 || !w || !ptgt || !qtgt) return fail(MPCR_EINVAL, "null argument");
  if (n < 0 || n > e->max_n) return fail(MPCR_EINVAL, "n=%d outside [0, max_n=%d]", n, e->max_n);
  if (int rc = check_layout(layout)) return rc;
  if (n == 0) return MPCR_OK;  // an empty batch: input / cost4 may be null (a zero-size tensor's data pointer)
  if (!input || !cost4) return fail(MPCR_EINVAL, "null argument");
  HIPCHK(hipSetDevice(e->device));
  hipStream_t st = (hipStream_t)stream;
  auto* key = reinterpret_cast<unsigned long long*>(best_key);
  const int nc = e->host.nctrl;
  Launch l;
  l.layout = layout;
  l.n = n;
  l.index_base = index_base;
  fill_par(l.par, nc, q0, w, ptgt, qtgt);
  if (flags & MPCR_F_DEVICE_PTRS) {
    l.in = input; l.cost4 = cost4; l.theta = theta; l.thetadot = thetadot; l.key = key; l.status = status;
    l.reset_key = (flags & MPCR_F_RESET_BEST) != 0;
    int rc = launch_rollout(e, l, st);
    if (rc) return rc;
    if (flags & MPCR_F_SYNC) HIPCHK(hipStreamSynchronize(st));
    return MPCR_OK;
  }
  if (int rc = stage_input(e, input, layout, n, st)) return rc;
  l.in = e->d_in; l.cost4 = e->d_cost; l.theta = theta ? e->d_theta : nullptr;
  l.thetadot = thetadot ? e->d_thetadot : nullptr; l.key = best_key ? e->d_key : nullptr;
  l.status = status ? e->d_status : nullptr; l.reset_key = true;
  int rc = launch_rollout(e, l, st);
  if (rc) return rc;
  HIPCHK(hipMemcpyAsync(cost4, e->d_cost, sizeof(float) * 4 * n, hipMemcpyDeviceToHost, st));
  if (theta) HIPCHK(hipMemcpyAsync(theta, e->d_theta, sizeof(float) * n * nc * e->H, hipMemcpyDeviceToHost, st));
  if (thetadot)
    HIPCHK(hipMemcpyAsync(thetadot, e->d_thetadot, sizeof(float) * n * nc * e->H, hipMemcpyDeviceToHost, st));
  if (best_key) HIPCHK(hipMemcpyAsync(best_key, e->d_key, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
  if (status) HIPCHK(hipMemcpyAsync(status, e->d_status, sizeof(int) * n, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return MPCR_OK;
}

// The shape a *_multi entry accepts: at least one problem of one candidate,
// all of them within the handle's max_n.
static int check_multi(int nprob, int n_per, int max_n) {
  if (nprob < 1 || n_per < 1) return fail(MPCR_EINVAL, "nprob=%d, n_per=%d: both must be >= 1", nprob, n_per);
  if ((long long)nprob * n_per > max_n)
    return fail(MPCR_EINVAL, "nprob=%d x n_per=%d exceeds max_n=%d", nprob, n_per, max_n);
  return MPCR_OK;
}

extern "C" int mpcr_state_layout(int* qpos, int* qvel, int* qacc_warmstart, int* qacc, int* eef) {
  if (qpos) *qpos = ST_QPOS;
  if (qvel) *qvel = ST_QVEL;
  if (qacc_warmstart) *qacc_warmstart = ST_QWS;
  if (qacc) *qacc = ST_QACC;
  if (eef) *eef = ST_EEF;
  return ST_N;
}

// Whether a model's controls can be replaced after its engine was built
// (a call's control block, mpcr_plant_set_ctrl): it has actuators, and the
// implicit integrator's D, built once, does not depend on them.
static int check_ctrl_model(const mpcr_model_t& h) {
  if (h.nu == 0) return fail(MPCR_EINVAL, "ctrl: the model has no actuators (nu = 0)");
  if (implicit_D_reads_ctrl(h))
    return fail(MPCR_EMODEL, "ctrl: an implicitfast model with a velocity-dependent actuator gain (gainprm[2] != 0) "
                             "keeps the controls it was built with: its D is derived once, at engine creation");
  return MPCR_OK;
}

// Whether a device model has a static collision geom: a row a geom-pose block
// (a call's, mpcr_plant_set_geom_poses') could replace.
static int check_geom_pose_model(const DevModel& d) {
  for (int i = 0; i < d.ngeom; i++)
    if (d.geom_body[i] < 0) return MPCR_OK;
  return fail(MPCR_EINVAL, "geom_pose: the model has no static collision geom");
}

// whether p is device memory on device d: what a kernel that runs there reads or writes
static bool device_memory(const void* p, int d) {
  hipPointerAttribute_t at;
  if (hipPointerGetAttributes(&at, p) == hipSuccess && at.type == hipMemoryTypeDevice && at.device == d) return true;
  (void)hipGetLastError();
  return false;
}

// A call's block per problem and, optionally, per step (StateArgs): `name` at
// p, addressed by `stem`_stride and `stem`_step_stride in floats, one unit of
// `unit` floats (named `unit_name`) per step.  align: bytes its rows are
// aligned to (0: no demand).  ctrl: nu floats; geom_pose: 8 ngeom, 16 bytes;
// target: a row of 8, 16 bytes; slot_w: nslot floats, 16 bytes, no step stride;
// step_w: 4 H floats (H contiguous rows of 4), 16 bytes, no step stride.
static int check_block(const mpcr_engine* e, const char* name, const char* stem, const float* p, int stride,
                       int step_stride, const char* unit_name, int unit, int align) {
  if (align && ((reinterpret_cast<uintptr_t>(p) & (align - 1)) || (stride & (align / 4 - 1)) ||
                (step_stride & (align / 4 - 1))))
    return fail(MPCR_EINVAL, "%s=%p, %s_stride=%d, %s_step_stride=%d: rows are %d-byte aligned (strides are "
                             "multiples of %d floats)",
                name, (const void*)p, stem, stride, stem, step_stride, align, align / 4);
  if (step_stride != 0 && step_stride < unit)
    return fail(MPCR_EINVAL, "%s_step_stride=%d: 0 (constant over the horizon) or at least %s=%d floats", stem,
                step_stride, unit_name, unit);
  const long long rows = step_stride ? (long long)step_stride * (e->H - 1) + unit : unit;  // floats one problem reads
  if (stride != 0 && stride < rows)
    return fail(MPCR_EINVAL, "%s_stride=%d: 0 (one block for every problem) or at least the %lld floats a problem "
                             "reads (%s=%d, %s_step_stride=%d, H=%d)",
                stem, stride, rows, unit_name, unit, stem, step_stride, e->H);
  // read by the kernel when it runs
  if (!device_memory(p, e->device))
    return fail(MPCR_EINVAL, "%s must be device memory on the engine's device %d", name, e->device);
  return MPCR_OK;
}

// Where every device-pointer rollout entry ends, its own checks made and the
// call described in l: l.nprob rollout problems of l.n candidates in all.
// The state blocks that are set are validated (a model that cannot take the
// block refuses first), then the launch and the sync.  One problem runs the
// one-problem kernels through any entry (prob_n = 0): the MULTI
// instantiations' problem lookup is paid only where there is one to make.
static int rollout_call(mpcr_engine* e, Launch& l, int flags, void* stream) {
  StateArgs& s = l.blk.st;
  if (s.start && s.start_stride != 0 && s.start_stride < ST_N)
    return fail(MPCR_EINVAL, "start_stride=%d: 0 (one block for every problem) or at least the block's %d floats",
                s.start_stride, (int)ST_N);
  if (s.ctrl) {
    if (int rc = check_ctrl_model(e->host)) return rc;
    if (int rc = check_block(e, "ctrl", "ctrl", s.ctrl, s.ctrl_stride, s.ctrl_step_stride, "nu", e->host.nu, 0))
      return rc;
  }
  if (s.geom_pose) {
    if (int rc = check_geom_pose_model(e->dev)) return rc;
    if (int rc = check_block(e, "geom_pose", "geom", s.geom_pose, s.geom_stride, s.geom_step_stride, "8 ngeom",
                             8 * e->dev.ngeom, 16))
      return rc;
  }
  // a block that is not set has no strides
  if (!s.start) s.start_stride = 0;
  if (!s.ctrl) s.ctrl_stride = s.ctrl_step_stride = 0;
  if (!s.geom_pose) s.geom_stride = s.geom_step_stride = 0;
  TargetArgs& tg = l.blk.tg;
  if (tg.target) {
    if (int rc = check_block(e, "target", "target", tg.target, tg.stride, tg.step_stride, "a target row", 8, 16))
      return rc;
    // the kernel parks a problem's offset as a count of 4-float quads in 32 bits
    if ((((long long)(l.nprob - 1) * tg.stride) >> 2) > 0xffffffffll)
      return fail(MPCR_EINVAL, "target_stride=%d x nprob=%d: a problem's offset exceeds 2^34 floats", tg.stride,
                  l.nprob);
  } else {
    tg.stride = tg.step_stride = 0;
  }
  SlotWArgs& sw = l.sw;
  if (sw.slot_w) {
    if (e->host.nslot == 0) return fail(MPCR_EINVAL, "slot_w: the model has no robot-masked contact slot (nslot = 0)");
    if (sw.stride < 0) return fail(MPCR_EINVAL, "slot_w_stride=%d: 0 or at least nslot=%d", sw.stride, e->host.nslot);
    if (int rc = check_block(e, "slot_w", "slot_w", sw.slot_w, sw.stride, 0, "nslot", e->host.nslot, 16)) return rc;
  } else {
    sw.stride = 0;
  }
  sw.pad_ = 0;
  // (a model without slots is fine: the pose columns price the dual arm too)
  StepWArgs& stw = l.stw;
  if (stw.step_w) {
    if (int rc = check_block(e, "step_w", "step_w", stw.step_w, stw.stride, 0, "4 H", 4 * e->H, 16)) return rc;
    if (!step_w_stride_ok(stw.stride, e->H))  // (check_block's rules, restated where a host program can test them)
      return fail(MPCR_EINVAL, "step_w_stride=%d: 0 or a multiple of 4 floats at least 4 H=%d", stw.stride, 4 * e->H);
  } else {
    stw.stride = 0;
  }
  stw.pad_ = 0;
  if (int rc = check_layout(l.layout)) return rc;
  if (!l.in || !l.dpar || !l.cost4) return fail(MPCR_EINVAL, "null argument");
  HIPCHK(hipSetDevice(e->device));
  hipStream_t st = (hipStream_t)stream;
  l.prob_n = l.nprob > 1 ? l.n / l.nprob : 0;
  l.reset_key = (flags & MPCR_F_RESET_BEST) != 0;
  if (int rc = launch_rollout(e, l, st)) return rc;
  if (flags & MPCR_F_SYNC) HIPCHK(hipStreamSynchronize(st));
  return MPCR_OK;
}

extern "C" int mpcr_rollout_cost_dp(mpcr_engine* e, const float* input, int layout, int n, const float* params,
                                    float* cost4, float* theta, float* thetadot, uint64_t* best_key, int index_base,
                                    int* status, int flags, void* stream) {
  if (!e) return fail(MPCR_EINVAL, "null argument");
  if (n < 0 || n > e->max_n) return fail(MPCR_EINVAL, "n=%d outside [0, max_n=%d]", n, e->max_n);
  if (n == 0) return check_layout(layout);  // an empty batch: the buffers may be null
  Launch l;
  l.in = input; l.layout = layout; l.n = n; l.dpar = params; l.index_base = index_base;
  l.cost4 = cost4; l.theta = theta; l.thetadot = thetadot; l.status = status;
  l.key = reinterpret_cast<unsigned long long*>(best_key);
  return rollout_call(e, l, flags, stream);
}

extern "C" int mpcr_rollout_cost_multi(mpcr_engine* e, const float* input, int layout, int nprob, int n_per,
                                       const float* params, float* cost4, float* theta, float* thetadot,
                                       uint64_t* best_keys, int index_base, int* status, int flags, void* stream) {
  if (!e) return fail(MPCR_EINVAL, "null argument");
  if (!(flags & MPCR_F_DEVICE_PTRS)) return fail(MPCR_EINVAL, "mpcr_rollout_cost_multi takes device pointers");
  if (int rc = check_multi(nprob, n_per, e->max_n)) return rc;
  Launch l;
  l.in = input; l.layout = layout; l.nprob = nprob; l.n = nprob * n_per; l.dpar = params; l.index_base = index_base;
  l.cost4 = cost4; l.theta = theta; l.thetadot = thetadot; l.status = status;
  l.key = reinterpret_cast<unsigned long long*>(best_keys);
  return rollout_call(e, l, flags, stream);
}

extern "C" int mpcr_rollout_cost_stepw(mpcr_engine* e, const float* input, int layout, int nprob, int n_per,
                                       const float* params, const float* start, int start_stride, float* final_state,
                                       const float* ctrl, int ctrl_stride, int ctrl_step_stride,
                                       const float* geom_pose, int geom_stride, int geom_step_stride,
                                       const float* target, int target_stride, int target_step_stride,
                                       const float* slot_w, int slot_w_stride, const float* step_w, int step_w_stride,
                                       float* cost4, float* theta, float* thetadot, uint64_t* best_keys,
                                       int index_base, int* status, int flags, void* stream) {
  if (!e) return fail(MPCR_EINVAL, "null argument");
  if (!(flags & MPCR_F_DEVICE_PTRS)) return fail(MPCR_EINVAL, "mpcr_rollout_cost_state takes device pointers");
  if (int rc = check_multi(nprob, n_per, e->max_n)) return rc;
  Launch l;
  l.in = input; l.layout = layout; l.nprob = nprob; l.n = nprob * n_per; l.dpar = params; l.index_base = index_base;
  l.cost4 = cost4; l.theta = theta; l.thetadot = thetadot; l.status = status;
  l.key = reinterpret_cast<unsigned long long*>(best_keys);
  l.blk.st.start = start; l.blk.st.start_stride = start_stride; l.blk.st.final_state = final_state;
  l.blk.st.ctrl = ctrl; l.blk.st.ctrl_stride = ctrl_stride; l.blk.st.ctrl_step_stride = ctrl_step_stride;
  l.blk.st.geom_pose = geom_pose; l.blk.st.geom_stride = geom_stride; l.blk.st.geom_step_stride = geom_step_stride;
  l.blk.tg.target = target; l.blk.tg.stride = target_stride; l.blk.tg.step_stride = target_step_stride;
  l.sw.slot_w = slot_w; l.sw.stride = slot_w_stride;
  l.stw.step_w = step_w; l.stw.stride = step_w_stride;
  return rollout_call(e, l, flags, stream);
}

extern "C" int mpcr_rollout_cost_slotw(mpcr_engine* e, const float* input, int layout, int nprob, int n_per,
                                       const float* params, const float* start, int start_stride, float* final_state,
                                       const float* ctrl, int ctrl_stride, int ctrl_step_stride,
                                       const float* geom_pose, int geom_stride, int geom_step_stride,
                                       const float* target, int target_stride, int target_step_stride,
                                       const float* slot_w, int slot_w_stride, float* cost4, float* theta,
                                       float* thetadot, uint64_t* best_keys, int index_base, int* status, int flags,
                                       void* stream) {
  return mpcr_rollout_cost_stepw(e, input, layout, nprob, n_per, params, start, start_stride, final_state, ctrl,
                                 ctrl_stride, ctrl_step_stride, geom_pose, geom_stride, geom_step_stride, target,
                                 target_stride, target_step_stride, slot_w, slot_w_stride, nullptr, 0, cost4, theta,
                                 thetadot, best_keys, index_base, status, flags, stream);
}

extern "C" int mpcr_rollout_cost_target(mpcr_engine* e, const float* input, int layout, int nprob, int n_per,
                                        const float* params, const float* start, int start_stride, float* final_state,
                                        const float* ctrl, int ctrl_stride, int ctrl_step_stride,
                                        const float* geom_pose, int geom_stride, int geom_step_stride,
                                        const float* target, int target_stride, int target_step_stride, float* cost4,
                                        float* theta, float* thetadot, uint64_t* best_keys, int index_base,
                                        int* status, int flags, void* stream) {
  return mpcr_rollout_cost_slotw(e, input, layout, nprob, n_per, params, start, start_stride, final_state, ctrl,
                                 ctrl_stride, ctrl_step_stride, geom_pose, geom_stride, geom_step_stride, target,
                                 target_stride, target_step_stride, nullptr, 0, cost4, theta, thetadot, best_keys,
                                 index_base, status, flags, stream);
}

extern "C" int mpcr_rollout_cost_world(mpcr_engine* e, const float* input, int layout, int nprob, int n_per,
                                       const float* params, const float* start, int start_stride, float* final_state,
                                       const float* ctrl, int ctrl_stride, int ctrl_step_stride,
                                       const float* geom_pose, int geom_stride, int geom_step_stride, float* cost4,
                                       float* theta, float* thetadot, uint64_t* best_keys, int index_base, int* status,
                                       int flags, void* stream) {
  return mpcr_rollout_cost_target(e, input, layout, nprob, n_per, params, start, start_stride, final_state, ctrl,
                                  ctrl_stride, ctrl_step_stride, geom_pose, geom_stride, geom_step_stride, nullptr, 0,
                                  0, cost4, theta, thetadot, best_keys, index_base, status, flags, stream);
}

// the shape mpcr_scenario_reduce and mpcr_rollout_cost_scenarios accept
static int check_scenarios(int nprob, int nscen, int n_per, int worst, int max_n) {
  if (nscen < 1 || nscen > SCEN_MAX) return fail(MPCR_EINVAL, "nscen=%d outside [1, %d]", nscen, SCEN_MAX);
  if (worst < 1 || worst > nscen) return fail(MPCR_EINVAL, "worst=%d outside [1, nscen=%d]", worst, nscen);
  if (nprob < 1 || n_per < 1) return fail(MPCR_EINVAL, "nprob=%d, n_per=%d: both must be >= 1", nprob, n_per);
  if ((long long)nprob * nscen * n_per > max_n)
    return fail(MPCR_EINVAL, "nprob=%d x nscen=%d x n_per=%d exceeds max_n=%d", nprob, nscen, n_per, max_n);
  if (nprob > 65535) return fail(MPCR_EINVAL, "nprob=%d exceeds the grid's 65535", nprob);
  return MPCR_OK;
}

// cost4_scen and cost4 are read / written when the kernel runs: device memory
// on the engine's device, rows 16-byte aligned
static int check_cost_rows(const mpcr_engine* e, const void* p, const char* name) {
  if (!device_memory(p, e->device))
    return fail(MPCR_EINVAL, "%s must be device memory on the engine's device %d", name, e->device);
  if (reinterpret_cast<uintptr_t>(p) & 15) return fail(MPCR_EINVAL, "%s=%p: rows are 16-byte aligned", name, p);
  return MPCR_OK;
}

extern "C" int mpcr_scenario_reduce(mpcr_engine* e, const float* cost4_scen, int nprob, int nscen, int n_per, int worst,
                                    float* cost4, uint64_t* best_keys, int index_base, int flags, void* stream) {
  if (!e || !cost4_scen || !cost4) return fail(MPCR_EINVAL, "null argument");
  if (!(flags & MPCR_F_DEVICE_PTRS)) return fail(MPCR_EINVAL, "mpcr_scenario_reduce takes device pointers");
  if (int rc = check_scenarios(nprob, nscen, n_per, worst, e->max_n)) return rc;
  if (int rc = check_cost_rows(e, cost4_scen, "cost4_scen")) return rc;
  if (int rc = check_cost_rows(e, cost4, "cost4")) return rc;
  HIPCHK(hipSetDevice(e->device));
  hipStream_t st = (hipStream_t)stream;
  auto* keys = reinterpret_cast<unsigned long long*>(best_keys);
  if (keys && (flags & MPCR_F_RESET_BEST)) hipLaunchKernelGGL(fill_u64, dim3(nprob), dim3(1), 0, st, keys, ~0ull);
  hipLaunchKernelGGL(scenario_reduce_kernel, dim3((n_per + SCEN_BLOCK - 1) / SCEN_BLOCK, nprob), dim3(SCEN_BLOCK), 0,
                     st, reinterpret_cast<const float4*>(cost4_scen), nscen, n_per, worst,
                     reinterpret_cast<float4*>(cost4), keys, index_base);
  HIPCHK(hipGetLastError());
  if (flags & MPCR_F_SYNC) HIPCHK(hipStreamSynchronize(st));
  return MPCR_OK;
}

extern "C" int mpcr_rollout_cost_scenarios_stepw(mpcr_engine* e, const float* input, int layout, int nprob, int nscen,
                                                 int worst, int n_per, const float* params, const float* start,
                                                 int start_stride, float* final_state, const float* ctrl,
                                                 int ctrl_stride, int ctrl_step_stride, const float* geom_pose,
                                                 int geom_stride, int geom_step_stride, const float* target,
                                                 int target_stride, int target_step_stride, const float* slot_w,
                                                 int slot_w_stride, const float* step_w, int step_w_stride,
                                                 float* cost4_scen, float* cost4, float* theta, float* thetadot,
                                                 uint64_t* best_keys, int index_base, int* status, int flags,
                                                 void* stream) {
  if (!e) return fail(MPCR_EINVAL, "null argument");
  if (!(flags & MPCR_F_DEVICE_PTRS)) return fail(MPCR_EINVAL, "mpcr_rollout_cost_scenarios takes device pointers");
  if (int rc = check_scenarios(nprob, nscen, n_per, worst, e->max_n)) return rc;
  if (!cost4_scen) return fail(MPCR_EINVAL, "null argument");
  if (best_keys && !cost4) return fail(MPCR_EINVAL, "best_keys come from the reduction: they need cost4");
  if (int rc = check_cost_rows(e, cost4_scen, "cost4_scen")) return rc;
  if (cost4)
    if (int rc = check_cost_rows(e, cost4, "cost4")) return rc;
  // the rollout: nprob nscen ordinary problems, every nscen of them in a row the scenarios of one planning
  // problem (input, theta and thetadot hold nprob n_per rows; no keys: the reduction's), then the fold
  Launch l;
  l.in = input; l.layout = layout; l.nprob = nprob * nscen; l.n = l.nprob * n_per; l.dpar = params;
  l.index_base = index_base; l.blk.nscen = nscen > 1 ? nscen : 0;
  l.cost4 = cost4_scen; l.theta = theta; l.thetadot = thetadot; l.status = status;
  l.blk.st.start = start; l.blk.st.start_stride = start_stride; l.blk.st.final_state = final_state;
  l.blk.st.ctrl = ctrl; l.blk.st.ctrl_stride = ctrl_stride; l.blk.st.ctrl_step_stride = ctrl_step_stride;
  l.blk.st.geom_pose = geom_pose; l.blk.st.geom_stride = geom_stride; l.blk.st.geom_step_stride = geom_step_stride;
  l.blk.tg.target = target; l.blk.tg.stride = target_stride; l.blk.tg.step_stride = target_step_stride;
  l.sw.slot_w = slot_w; l.sw.stride = slot_w_stride;
  l.stw.step_w = step_w; l.stw.stride = step_w_stride;
  if (int rc = rollout_call(e, l, flags & ~(MPCR_F_SYNC | MPCR_F_RESET_BEST), stream)) return rc;
  if (cost4)
    return mpcr_scenario_reduce(e, cost4_scen, nprob, nscen, n_per, worst, cost4, best_keys, index_base, flags,
                                stream);
  if (flags & MPCR_F_SYNC) HIPCHK(hipStreamSynchronize((hipStream_t)stream));
  return MPCR_OK;
}

extern "C" int mpcr_rollout_cost_scenarios_slotw(mpcr_engine* e, const float* input, int layout, int nprob, int nscen,
                                                 int worst, int n_per, const float* params, const float* start,
                                                 int start_stride, float* final_state, const float* ctrl,
                                                 int ctrl_stride, int ctrl_step_stride, const float* geom_pose,
                                                 int geom_stride, int geom_step_stride, const float* target,
                                                 int target_stride, int target_step_stride, const float* slot_w,
                                                 int slot_w_stride, float* cost4_scen, float* cost4, float* theta,
                                                 float* thetadot, uint64_t* best_keys, int index_base, int* status,
                                                 int flags, void* stream) {
  return mpcr_rollout_cost_scenarios_stepw(e, input, layout, nprob, nscen, worst, n_per, params, start, start_stride,
                                           final_state, ctrl, ctrl_stride, ctrl_step_stride, geom_pose, geom_stride,
                                           geom_step_stride, target, target_stride, target_step_stride, slot_w,
                                           slot_w_stride, nullptr, 0, cost4_scen, cost4, theta, thetadot, best_keys,
                                           index_base, status, flags, stream);
}

extern "C" int mpcr_rollout_cost_scenarios_target(mpcr_engine* e, const float* input, int layout, int nprob, int nscen,
                                                  int worst, int n_per, const float* params, const float* start,
                                                  int start_stride, float* final_state, const float* ctrl,
                                                  int ctrl_stride, int ctrl_step_stride, const float* geom_pose,
                                                  int geom_stride, int geom_step_stride, const float* target,
                                                  int target_stride, int target_step_stride, float* cost4_scen,
                                                  float* cost4, float* theta, float* thetadot, uint64_t* best_keys,
                                                  int index_base, int* status, int flags, void* stream) {
  return mpcr_rollout_cost_scenarios_slotw(e, input, layout, nprob, nscen, worst, n_per, params, start, start_stride,
                                           final_state, ctrl, ctrl_stride, ctrl_step_stride, geom_pose, geom_stride,
                                           geom_step_stride, target, target_stride, target_step_stride, nullptr, 0,
                                           cost4_scen, cost4, theta, thetadot, best_keys, index_base, status, flags,
                                           stream);
}

extern "C" int mpcr_rollout_cost_scenarios(mpcr_engine* e, const float* input, int layout, int nprob, int nscen,
                                           int worst, int n_per, const float* params, const float* start,
                                           int start_stride, float* final_state, const float* ctrl, int ctrl_stride,
                                           int ctrl_step_stride, const float* geom_pose, int geom_stride,
                                           int geom_step_stride, float* cost4_scen, float* cost4, float* theta,
                                           float* thetadot, uint64_t* best_keys, int index_base, int* status,
                                           int flags, void* stream) {
  return mpcr_rollout_cost_scenarios_target(e, input, layout, nprob, nscen, worst, n_per, params, start, start_stride,
                                            final_state, ctrl, ctrl_stride, ctrl_step_stride, geom_pose, geom_stride,
                                            geom_step_stride, nullptr, 0, 0, cost4_scen, cost4, theta, thetadot,
                                            best_keys, index_base, status, flags, stream);
}

extern "C" int mpcr_rollout_cost_ctrl(mpcr_engine* e, const float* input, int layout, int nprob, int n_per,
                                      const float* params, const float* start, int start_stride, float* final_state,
                                      const float* ctrl, int ctrl_stride, int ctrl_step_stride, float* cost4,
                                      float* theta, float* thetadot, uint64_t* best_keys, int index_base, int* status,
                                      int flags, void* stream) {
  return mpcr_rollout_cost_world(e, input, layout, nprob, n_per, params, start, start_stride, final_state, ctrl,
                                 ctrl_stride, ctrl_step_stride, nullptr, 0, 0, cost4, theta, thetadot, best_keys,
                                 index_base, status, flags, stream);
}

extern "C" int mpcr_rollout_cost_state(mpcr_engine* e, const float* input, int layout, int nprob, int n_per,
                                       const float* params, const float* start, int start_stride, float* final_state,
                                       float* cost4, float* theta, float* thetadot, uint64_t* best_keys,
                                       int index_base, int* status, int flags, void* stream) {
  return mpcr_rollout_cost_ctrl(e, input, layout, nprob, n_per, params, start, start_stride, final_state, nullptr, 0, 0,
                                cost4, theta, thetadot, best_keys, index_base, status, flags, stream);
}

// ---------------------------------------------------------------------------
// closed-loop plant: one environment stepped by the same kernel (n = 1, H = 1,
// qvel[:nctrl] overridden like SBP/mpc_planner.py:179-180), state resident on
// the device between calls

struct mpcr_plant {
  mpcr_engine* e = nullptr;
  DevBufs mem;
  float* d_state = nullptr;  // ST_N floats (rollout.hip layout)
  float* d_in = nullptr;     // nctrl joint velocities
  float* d_cost = nullptr;   // unused cost4 of the single "candidate"
  float h_state[ST_N] = {};
};

extern "C" void mpcr_plant_free(mpcr_plant* p) {
  if (!p) return;
  mpcr_engine_free(p->e);
  delete p;
}

extern "C" int mpcr_plant_create(const mpcr_model* m, int device, mpcr_plant** out) {
  if (!m || !out) return fail(MPCR_EINVAL, "null argument");
  const float pdot[1] = {0.f};
  auto* p = new mpcr_plant;
  int rc = mpcr_engine_create(m, device, 1, 1, pdot, 1, &p->e);
  if (rc) { delete p; return rc; }
  const mpcr_model_t& h = p->e->host;
  for (int i = 0; i < h.nq; i++) p->h_state[ST_QPOS + i] = (float)h.qpos_init[i];
  for (int i = 0; i < h.nv; i++) p->h_state[ST_QVEL + i] = (float)h.qvel_init[i];
  p->d_state = p->mem.alloc<float>(ST_N, p->h_state, ST_N);
  p->d_in = p->mem.alloc<float>(DX_NCTRL);
  p->d_cost = p->mem.alloc<float>(4);
  if (int rc = p->mem.rc) {
    mpcr_plant_free(p);
    return fail(rc, "%s", rc == MPCR_ENOMEM ? "device allocation failed" : "state upload failed");
  }
  *out = p;
  return MPCR_OK;
}

extern "C" int mpcr_plant_set_state(mpcr_plant* p, const double* qpos, const double* qvel,
                                    const double* qacc_warmstart) {
  if (!p) return fail(MPCR_EINVAL, "null plant");
  HIPCHK(hipSetDevice(p->e->device));
  const mpcr_model_t& h = p->e->host;
  HIPCHK(hipMemcpy(p->h_state, p->d_state, sizeof(float) * ST_N, hipMemcpyDeviceToHost));
  if (qpos)
    for (int i = 0; i < h.nq; i++) p->h_state[ST_QPOS + i] = (float)qpos[i];
  if (qvel)
    for (int i = 0; i < h.nv; i++) p->h_state[ST_QVEL + i] = (float)qvel[i];
  if (qacc_warmstart)
    for (int i = 0; i < h.nv; i++) p->h_state[ST_QWS + i] = (float)qacc_warmstart[i];
  HIPCHK(hipMemcpy(p->d_state, p->h_state, sizeof(float) * ST_N, hipMemcpyHostToDevice));
  // a new state starts a new trajectory: the hull-climb starts the plant
  // keeps across steps (like a rollout's, and the oracle's) start over
  HIPCHK(hipMemset(p->e->d_hints, 0xff, sizeof(short) * 2 * (p->e->wide ? SmemW::NHINT : 1)));
  return MPCR_OK;
}

extern "C" int mpcr_plant_get_state(mpcr_plant* p, double* qpos, double* qvel, double* qacc, double* eef) {
  if (!p) return fail(MPCR_EINVAL, "null plant");
  HIPCHK(hipSetDevice(p->e->device));
  const mpcr_model_t& h = p->e->host;
  HIPCHK(hipMemcpy(p->h_state, p->d_state, sizeof(float) * ST_N, hipMemcpyDeviceToHost));
  if (qpos)
    for (int i = 0; i < h.nq; i++) qpos[i] = p->h_state[ST_QPOS + i];
  if (qvel)
    for (int i = 0; i < h.nv; i++) qvel[i] = p->h_state[ST_QVEL + i];
  if (qacc)
    for (int i = 0; i < h.nv; i++) qacc[i] = p->h_state[ST_QACC + i];
  if (eef)
    for (int i = 0; i < 7; i++) eef[i] = p->h_state[ST_EEF + i];
  return MPCR_OK;
}

// the plant's block (mpcr_state_layout) to device memory, in stream order: a
// planner's start state (mpcr_rollout_cost_state) with no host round trip
extern "C" int mpcr_plant_copy_state(mpcr_plant* p, float* d_dst, void* stream) {
  if (!p || !d_dst) return fail(MPCR_EINVAL, "null argument");
  HIPCHK(hipSetDevice(p->e->device));
  // the copy runs on the plant's device: the destination must live there
  if (!device_memory(d_dst, p->e->device))
    return fail(MPCR_EINVAL, "d_dst must be device memory on the plant's device %d", p->e->device);
  HIPCHK(hipMemcpyAsync(d_dst, p->d_state, sizeof(float) * ST_N, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return MPCR_OK;
}

// The plant's controls: clamped here as build_dev_model clamps the model's
// own, written into the plant's engine's device copy of act_gain[a][3] (the
// plant owns that engine, and runs the kernels that read the control there).
// NULL: the model's own again.
extern "C" int mpcr_plant_set_ctrl(mpcr_plant* p, const double* ctrl) {
  if (!p) return fail(MPCR_EINVAL, "null plant");
  mpcr_engine* e = p->e;
  const mpcr_model_t& h = e->host;
  if (int rc = check_ctrl_model(h)) return rc;
  HIPCHK(hipSetDevice(e->device));
  for (int a = 0; a < h.nu; a++) e->dev.act_gain[a][3] = clamped_ctrl(h, a, ctrl ? ctrl[a] : h.act_ctrl[a]);
  static_assert(sizeof(e->dev.act_gain) == sizeof(float) * 4 * DX_NU, "act_gain rows");
  HIPCHK(hipMemcpy(reinterpret_cast<char*>(e->d_model) + offsetof(DevModel, act_gain), e->dev.act_gain,
                   sizeof(e->dev.act_gain), hipMemcpyHostToDevice));
  return MPCR_OK;
}

// The plant's static geom poses: the static rows of a geom-pose block written
// into the plant's engine's device copy of geom_pos / geom_quat, which the
// kernels that step the plant read.  NULL: the model's own again.
extern "C" int mpcr_plant_set_geom_poses(mpcr_plant* p, const float* block) {
  if (!p) return fail(MPCR_EINVAL, "null plant");
  mpcr_engine* e = p->e;
  if (int rc = check_geom_pose_model(e->dev)) return rc;
  float own[8 * DX_NG];
  if (!block) {
    if (model_geom_poses(e->host, own, nullptr, nullptr) != e->dev.ngeom) return fail(MPCR_EMODEL, "geom count");
    block = own;
  }
  HIPCHK(hipSetDevice(e->device));
  for (int i = 0; i < e->dev.ngeom; i++) {
    if (e->dev.geom_body[i] >= 0) continue;
    for (int k = 0; k < 3; k++) e->dev.geom_pos[i][k] = block[8 * i + k];
    for (int k = 0; k < 4; k++) e->dev.geom_quat[i][k] = block[8 * i + 4 + k];
  }
  static_assert(offsetof(DevModel, geom_quat) == offsetof(DevModel, geom_pos) + sizeof(e->dev.geom_pos),
                "geom_pos | geom_quat adjacent");
  HIPCHK(hipMemcpy(reinterpret_cast<char*>(e->d_model) + offsetof(DevModel, geom_pos), e->dev.geom_pos,
                   sizeof(e->dev.geom_pos) + sizeof(e->dev.geom_quat), hipMemcpyHostToDevice));
  return MPCR_OK;
}

// The plant's one-candidate launch on st: the joint velocities v (host, nctrl;
// the caller syncs before v goes) staged as the input, the state block
// stepped in place -- plant = 1: forward only, 3: a committed step
// (RolloutArgs::plant) -- with a zero parameter block, dbg as given.
static int plant_launch(mpcr_plant* p, const float* v, int plant, float* dbg, hipStream_t st) {
  mpcr_engine* e = p->e;
  const int nc = e->host.nctrl;
  HIPCHK(hipMemcpyAsync(p->d_in, v, sizeof(float) * nc, hipMemcpyHostToDevice, st));
  Launch l;
  l.layout = MPCR_LAYOUT_THETADOT; l.n = 1; l.in = p->d_in; l.cost4 = p->d_cost;
  l.state = p->d_state; l.plant = plant; l.dbg = dbg;
  const double q0[DX_NCTRL] = {};
  const float w[3] = {0.f, 0.f, 0.f}, pt[3] = {0.f, 0.f, 0.f}, qt[4] = {1.f, 0.f, 0.f, 0.f};
  fill_par(l.par, nc, q0, w, pt, qt);
  return launch_rollout(e, l, st);
}

// commit = 0: mj_forward (qacc and the eef pose of the current state, nothing
// advanced; qvel_ctrl ignored); commit = 1: mj_step with qvel[:nctrl] =
// qvel_ctrl (NULL keeps the current joint velocities)
extern "C" int mpcr_plant_step(mpcr_plant* p, const double* qvel_ctrl, int commit, void* stream) {
  if (!p) return fail(MPCR_EINVAL, "null plant");
  mpcr_engine* e = p->e;
  HIPCHK(hipSetDevice(e->device));
  hipStream_t st = (hipStream_t)stream;
  const int nc = e->host.nctrl;
  float v[DX_NCTRL] = {};
  if (!commit || !qvel_ctrl) {
    HIPCHK(hipMemcpyAsync(p->h_state, p->d_state, sizeof(float) * ST_N, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    for (int k = 0; k < nc; k++) v[k] = p->h_state[ST_QVEL + e->host.ctrl_dofadr[k]];
  } else {
    for (int k = 0; k < nc; k++) v[k] = (float)qvel_ctrl[k];
  }
  if (int rc = plant_launch(p, v, commit ? 3 : 1, nullptr, st)) return rc;
  HIPCHK(hipStreamSynchronize(st));
  return MPCR_OK;
}

// Debug/parity entry (not part of the stable ABI surface): one committed
// plant step (as mpcr_plant_step) that also copies the step's active
// contacts, constraint-row parameters, qacc_smooth and final qacc into
// dbg_host (mpcr_plant_dbg_size() floats; layout DBG_* of rollout.h, the
// oracle's oracle_step_debug writes the same).
extern "C" int mpcr_plant_dbg_size(void) { return DBG_N; }
extern "C" int mpcr_plant_step_debug(mpcr_plant* p, const double* qvel_ctrl, float* dbg_host, int mpr_pair) {
  if (!p || !qvel_ctrl || !dbg_host) return fail(MPCR_EINVAL, "bad debug step arguments");
  mpcr_engine* e = p->e;
  HIPCHK(hipSetDevice(e->device));
  const int nc = e->host.nctrl;
  float v[DX_NCTRL] = {};
  for (int k = 0; k < nc; k++) v[k] = (float)qvel_ctrl[k];
  DevBufs tmp;  // freed on every return
  float* d_dbg = tmp.alloc<float>(DBG_N);
  if (tmp.rc) return fail(tmp.rc, "device allocation failed");
  HIPCHK(hipMemset(d_dbg, 0, sizeof(float) * DBG_N));
  const float pf = (float)mpr_pair;  // the pair whose MPR the kernel traces (DBG_MPR), -1: none
  HIPCHK(hipMemcpy(d_dbg + DBG_MPR, &pf, sizeof(float), hipMemcpyHostToDevice));
  if (int rc = plant_launch(p, v, 3, d_dbg, nullptr)) return rc;
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(dbg_host, d_dbg, sizeof(float) * DBG_N, hipMemcpyDeviceToHost));
  return MPCR_OK;
}

// Debug/parity entry (not part of the stable ABI surface): host pointers,
// also returns the per-step eef pose (n x H x 7) and masked slot distances
// (n x H x nslot).
extern "C" int mpcr_rollout_trace(mpcr_engine* e, const float* input, int layout, int n, const double* q0,
                                  const float* w, const float* ptgt, const float* qtgt, float* cost4, float* theta,
                                  float* eef, float* slots) {
  if (!e || !input || !cost4 || n <= 0 || n > e->max_n) return fail(MPCR_EINVAL, "bad trace arguments");
  HIPCHK(hipSetDevice(e->device));
  const int nc = e->host.nctrl;
  const int nslot = e->host.nslot > 0 ? e->host.nslot : 1;
  DevBufs tmp;  // freed on every return
  float* d_eef = tmp.alloc<float>((size_t)n * e->H * 7);
  float* d_slots = tmp.alloc<float>((size_t)n * e->H * nslot);
  if (tmp.rc) return fail(tmp.rc, "device allocation failed");
  if (int rc = stage_input(e, input, layout, n, nullptr)) return rc;
  Launch l;
  l.layout = layout; l.n = n; l.in = e->d_in; l.cost4 = e->d_cost; l.theta = e->d_theta; l.status = e->d_status;
  l.trace_eef = d_eef; l.trace_slots = d_slots;
  fill_par(l.par, nc, q0, w, ptgt, qtgt);
  if (int rc = launch_rollout(e, l, nullptr)) return rc;
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(cost4, e->d_cost, sizeof(float) * 4 * n, hipMemcpyDeviceToHost));
  if (theta) HIPCHK(hipMemcpy(theta, e->d_theta, sizeof(float) * n * nc * e->H, hipMemcpyDeviceToHost));
  if (eef) HIPCHK(hipMemcpy(eef, d_eef, sizeof(float) * n * e->H * 7, hipMemcpyDeviceToHost));
  if (slots) HIPCHK(hipMemcpy(slots, d_slots, sizeof(float) * n * e->H * nslot, hipMemcpyDeviceToHost));
  return MPCR_OK;
}

#if defined(MPCR_PROFILE) || defined(MPCR_WAVETIME)
// the diagnostic launches' arguments: a host-parameter launch from the staged
// input with the counters in prof, as one launch (horizon segments off)
static int prof_args(const mpcr_engine* e, int layout, int n, const double* q0, const float* w, const float* ptgt,
                     const float* qtgt, unsigned long long* d_prof, RolloutArgs& a) {
  Launch l;
  l.layout = layout; l.n = n; l.in = e->d_in; l.cost4 = e->d_cost;
  fill_par(l.par, e->host.nctrl, q0, w, ptgt, qtgt);
  if (int rc = rollout_args(e, l, a)) return rc;
  a.prof = d_prof;
  a.seg_state = nullptr;
  a.seg = a.seg_min_n = 0;
  return MPCR_OK;
}
#endif

#ifdef MPCR_PROFILE
// diagnostic build only: per-phase s_memtime cycles summed over all waves
extern "C" int mpcr_rollout_profile(mpcr_engine* e, const float* input, int layout, int n, const double* q0,
                                    const float* w, const float* ptgt, const float* qtgt,
                                    unsigned long long* phases16 /* 64 slots: wave 0, wave 1 (WPC = 2) */) {
  HIPCHK(hipSetDevice(e->device));
  DevBufs tmp;  // freed on every return
  unsigned long long* d_prof = tmp.alloc<unsigned long long>(64);
  if (tmp.rc) return fail(tmp.rc, "device allocation failed");
  HIPCHK(hipMemset(d_prof, 0, 64 * sizeof(unsigned long long)));
  e->dev.prof = d_prof;  // wave-level counters for this launch only
  HIPCHK(hipMemcpy(e->d_model, &e->dev, sizeof(DevModel), hipMemcpyHostToDevice));
  if (int rc = stage_input(e, input, layout, n, nullptr)) return rc;
  RolloutArgs a;
  if (int rc = prof_args(e, layout, n, q0, w, ptgt, qtgt, d_prof, a)) return rc;
  rollout_launch(e->wide, a, (const DevModel*)e->d_model, n, nullptr);
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(phases16, d_prof, 64 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  e->dev.prof = nullptr;
  HIPCHK(hipMemcpy(e->d_model, &e->dev, sizeof(DevModel), hipMemcpyHostToDevice));
  return MPCR_OK;
}
#endif

#ifdef MPCR_WAVETIME
// diagnostic build only: per wave (start, end) on the 100 MHz clock, shader
// cycles, (XCC_ID << 32 | HW_ID) -- 4 u64 per candidate; then per candidate
// (line-search passes << 32 | Newton iterations, convex flush chunks)
extern "C" int mpcr_rollout_wavetime(mpcr_engine* e, const float* input, int layout, int n, const double* q0,
                                     const float* w, const float* ptgt, const float* qtgt, unsigned long long* out) {
  HIPCHK(hipSetDevice(e->device));
  DevBufs tmp;  // freed on every return
  unsigned long long* d_prof = tmp.alloc<unsigned long long>(6 * (size_t)n);
  if (tmp.rc) return fail(tmp.rc, "device allocation failed");
  HIPCHK(hipMemset(d_prof, 0, 6 * (size_t)n * sizeof(unsigned long long)));
  if (int rc = stage_input(e, input, layout, n, nullptr)) return rc;
  RolloutArgs a;
  if (int rc = prof_args(e, layout, n, q0, w, ptgt, qtgt, d_prof, a)) return rc;
  rollout_launch(e->wide, a, (const DevModel*)e->d_model, n, nullptr);
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(out, d_prof, 6 * (size_t)n * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  return MPCR_OK;
}
#endif

extern "C" void mpcr_best_key_decode(uint64_t key, int* idx, float* cost) {
  uint32_t hi = (uint32_t)(key >> 32);
  if (idx) *idx = (int)(uint32_t)(key & 0xffffffffu);
  if (cost) {
    if (hi == 0u) {
      *cost = NAN;
    } else {
      uint32_t u = (hi & 0x80000000u) ? (hi & 0x7fffffffu) : ~hi;
      float f;
      std::memcpy(&f, &u, 4);
      *cost = f;
    }
  }
}

extern "C" int mpcr_argmin(mpcr_engine* e, const float* cost, int stride, int n, int index_base, uint64_t* key_out,
                           int* idx_out, float* val_out, int flags, void* stream) {
  if (!e || !cost || n <= 0 || stride <= 0) return fail(MPCR_EINVAL, "bad argmin arguments");
  HIPCHK(hipSetDevice(e->device));
  hipStream_t st = (hipStream_t)stream;
  const float* dcost = cost;
  if (!(flags & MPCR_F_DEVICE_PTRS)) {
    if (n > e->max_n || stride > 4) return fail(MPCR_EINVAL, "host argmin limited to max_n x 4");
    HIPCHK(hipMemcpyAsync(e->d_cost, cost, sizeof(float) * (size_t)n * stride, hipMemcpyHostToDevice, st));
    dcost = e->d_cost;
  }
  unsigned long long* key = (flags & MPCR_F_DEVICE_PTRS) && key_out ? reinterpret_cast<unsigned long long*>(key_out)
                                                                    : e->d_key;
  hipLaunchKernelGGL(fill_u64, dim3(1), dim3(1), 0, st, key, ~0ull);
  int blocks = (n + 255) / 256;
  blocks = blocks > 1024 ? 1024 : blocks;
  hipLaunchKernelGGL(argmin_kernel, dim3(blocks), dim3(256), 0, st, dcost, stride, n, index_base, key);
  HIPCHK(hipGetLastError());
  if (idx_out || val_out || (key_out && !(flags & MPCR_F_DEVICE_PTRS))) {
    uint64_t k;
    HIPCHK(hipMemcpyAsync(&k, key, sizeof(k), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    mpcr_best_key_decode(k, idx_out, val_out);
    if (key_out && !(flags & MPCR_F_DEVICE_PTRS)) *key_out = k;
  } else if (flags & MPCR_F_SYNC) {
    HIPCHK(hipStreamSynchronize(st));
  }
  return MPCR_OK;
}

// mpcr_topk (nprob = 1) and mpcr_topk_multi: one workgroup per problem.
// Without MPCR_F_DEVICE_PTRS (mpcr_topk alone allows it) cost and idx_out are
// host arrays, staged through the engine's buffers.
static int topk(mpcr_engine* e, const float* cost, int stride, int nprob, int n_per, int k, int* idx_out, int flags,
                void* stream) {
  if (!e || !cost || !idx_out || stride <= 0 || n_per < 0) return fail(MPCR_EINVAL, "bad topk arguments");
  if (k < 0 || k > n_per || k > TOPK_MAX)
    return fail(MPCR_EINVAL, "k=%d outside [0, min(n=%d, %d)]", k, n_per, TOPK_MAX);
  if (k == 0) return MPCR_OK;
  HIPCHK(hipSetDevice(e->device));
  hipStream_t st = (hipStream_t)stream;
  const bool host = !(flags & MPCR_F_DEVICE_PTRS);
  if (host) {
    if (n_per > e->max_n || stride > 4) return fail(MPCR_EINVAL, "host topk limited to max_n x 4");
    HIPCHK(hipMemcpyAsync(e->d_cost, cost, sizeof(float) * (size_t)n_per * stride, hipMemcpyHostToDevice, st));
  }
  hipLaunchKernelGGL(topk_kernel, dim3(nprob), dim3(1024), 0, st, host ? e->d_cost : cost, stride, n_per, k,
                     host ? e->d_idx : idx_out);
  HIPCHK(hipGetLastError());
  if (host) HIPCHK(hipMemcpyAsync(idx_out, e->d_idx, sizeof(int) * k, hipMemcpyDeviceToHost, st));
  if (host || (flags & MPCR_F_SYNC)) HIPCHK(hipStreamSynchronize(st));
  return MPCR_OK;
}

extern "C" int mpcr_topk(mpcr_engine* e, const float* cost, int stride, int n, int k, int* idx_out, int flags,
                         void* stream) {
  return topk(e, cost, stride, 1, n, k, idx_out, flags, stream);
}

extern "C" int mpcr_topk_multi(mpcr_engine* e, const float* cost, int stride, int nprob, int n_per, int k,
                               int* idx_out, int flags, void* stream) {
  if (!e) return fail(MPCR_EINVAL, "bad topk arguments");
  if (!(flags & MPCR_F_DEVICE_PTRS)) return fail(MPCR_EINVAL, "mpcr_topk_multi takes device pointers");
  if (int rc = check_multi(nprob, n_per, e->max_n)) return rc;
  return topk(e, cost, stride, nprob, n_per, k, idx_out, flags, stream);
}

// ---------------------------------------------------------------------------
// CEM context (cem.hip kernels)

struct mpcr_cem {
  int device = 0, nd = 0, H = 0, max_n = 0;
  int nprob = 1;      // Cholesky factors d_LT holds (mpcr_cem_set_problems)
  int factored_n = 0; // problems the last factor call covered (0: none yet)
  float* d_X = nullptr;    // 3 x H x 12: Pdot, Pddot, P
  float* d_QT = nullptr;   // LD x LD
  float* d_QbT = nullptr;  // 5nd x LD
  float* d_LT = nullptr;   // LD x LD Cholesky factor (transposed, padded)
};

// get_Q_inv (SBP/mjx_planner.py:166-172 as restated by oracle/cem_np.q_inv):
// fp32 Gram blocks of kron(I, [X; -X]) promoted to fp64, fp64 KKT inverse.
static bool kkt_inverse(int nd, int H, const float* P, const float* Pd, const float* Pdd, std::vector<double>& Kinv) {
  const int nb = PJ_NB, nv = nd * nb, ne = 5 * nd, NK = nv + ne;
  std::vector<double> K((size_t)NK * NK, 0.0);
  const float* mats[3] = {Pd, Pdd, P};
  for (int a = 0; a < nb; a++)
    for (int b = 0; b < nb; b++) {
      double g = 0.0;
      for (int k = 0; k < 3; k++) {
        float s = 0.f;  // fp32 Gram entry over the 2H rows of [X; -X]
        for (int t = 0; t < H; t++) s += mats[k][t * nb + a] * mats[k][t * nb + b];
        for (int t = 0; t < H; t++) s += (-mats[k][t * nb + a]) * (-mats[k][t * nb + b]);
        g += (double)s;
      }
      for (int j = 0; j < nd; j++) K[(size_t)(j * nb + a) * NK + j * nb + b] = g + (a == b ? 1.0 : 0.0);
    }
  for (int j = 0; j < nd; j++)
    for (int c = 0; c < nb; c++) {
      const double rows[5] = {P[c], Pd[c], Pdd[c], Pd[(H - 1) * nb + c], Pdd[(H - 1) * nb + c]};
      for (int m = 0; m < 5; m++) {
        K[(size_t)(nv + j * 5 + m) * NK + j * nb + c] = rows[m];
        K[(size_t)(j * nb + c) * NK + nv + j * 5 + m] = rows[m];
      }
    }
  // Gauss-Jordan with partial pivoting
  Kinv.assign((size_t)NK * NK, 0.0);
  for (int i = 0; i < NK; i++) Kinv[(size_t)i * NK + i] = 1.0;
  for (int c = 0; c < NK; c++) {
    int piv = c;
    for (int r = c + 1; r < NK; r++)
      if (std::fabs(K[(size_t)r * NK + c]) > std::fabs(K[(size_t)piv * NK + c])) piv = r;
    if (K[(size_t)piv * NK + c] == 0.0) return false;
    if (piv != c)
      for (int q = 0; q < NK; q++) {
        std::swap(K[(size_t)c * NK + q], K[(size_t)piv * NK + q]);
        std::swap(Kinv[(size_t)c * NK + q], Kinv[(size_t)piv * NK + q]);
      }
    const double inv = 1.0 / K[(size_t)c * NK + c];
    for (int q = 0; q < NK; q++) { K[(size_t)c * NK + q] *= inv; Kinv[(size_t)c * NK + q] *= inv; }
    for (int r = 0; r < NK; r++) {
      if (r == c) continue;
      const double f = K[(size_t)r * NK + c];
      if (f == 0.0) continue;
      for (int q = 0; q < NK; q++) {
        K[(size_t)r * NK + q] -= f * K[(size_t)c * NK + q];
        Kinv[(size_t)r * NK + q] -= f * Kinv[(size_t)c * NK + q];
      }
    }
  }
  return true;
}

extern "C" int mpcr_cem_create(int device, int num_dof, int horizon, int nbasis, const double* P, const double* Pdot,
                               const double* Pddot, const double* qinv, int max_n, mpcr_cem** out) {
  if (!out || !P || !Pdot || !Pddot || max_n <= 0 || horizon < 2) return fail(MPCR_EINVAL, "bad cem arguments");
  if (nbasis != PJ_NB) return fail(MPCR_EINVAL, "nbasis=%d: the CEM kernels are built for order-10 (11)", nbasis);
  if (num_dof < 1 || num_dof > PJ_MAXD) return fail(MPCR_EINVAL, "num_dof=%d outside [1, %d]", num_dof, PJ_MAXD);
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(MPCR_ENODEV, "no HIP device");
  if (device < 0 || device >= ndev) return fail(MPCR_ENODEV, "device %d out of range (%d)", device, ndev);
  HIPCHK(hipSetDevice(device));
  hipDeviceProp_t prop;
  HIPCHK(hipGetDeviceProperties(&prop, device));
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail(MPCR_ENODEV, "device %d is %s; libmpcr is built for gfx950 only", device, prop.gcnArchName);
  const int nd = num_dof, H = horizon, nb = PJ_NB, nv = nd * nb, ne = 5 * nd, NK = nv + ne, LD = nd * PJ_BLK;
  {
    // sample_project_kernel stages the constraint rows X (3 x H x 12) and the
    // candidates' rows in LDS (mpcr_cem_sample_project): refuse a horizon
    // whose image exceeds the device's per-workgroup LDS
    const int cpw = PJ_CPW_LARGE > PJ_CPW_SMALL ? PJ_CPW_LARGE : PJ_CPW_SMALL;
    const size_t lds = sizeof(float) * (cpw * (nd * PJ_BLK + 4) + 3 * (size_t)H * PJ_BLK);
    if (lds > prop.sharedMemPerBlock)
      return fail(MPCR_EINVAL, "horizon=%d: the projection kernel's LDS image (%zu B) exceeds the device's %zu B per "
                  "workgroup", H, lds, (size_t)prop.sharedMemPerBlock);
  }
  std::vector<float> Pf((size_t)H * nb), Pdf((size_t)H * nb), Pddf((size_t)H * nb);
  for (int i = 0; i < H * nb; i++) { Pf[i] = (float)P[i]; Pdf[i] = (float)Pdot[i]; Pddf[i] = (float)Pddot[i]; }
  std::vector<double> Kinv;
  if (qinv) {
    Kinv.assign(qinv, qinv + (size_t)NK * NK);
  } else if (!kkt_inverse(nd, H, Pf.data(), Pdf.data(), Pddf.data(), Kinv)) {
    return fail(MPCR_EINVAL, "singular KKT matrix");
  }
  std::vector<float> X((size_t)3 * H * PJ_BLK, 0.f), QT((size_t)LD * LD, 0.f), QbT((size_t)ne * LD, 0.f);
  const float* mats[3] = {Pdf.data(), Pddf.data(), Pf.data()};
  for (int k = 0; k < 3; k++)
    for (int t = 0; t < H; t++)
      for (int c = 0; c < nb; c++) X[((size_t)k * H + t) * PJ_BLK + c] = mats[k][t * nb + c];
  auto pad = [&](int i) { return (i / nb) * PJ_BLK + i % nb; };
  for (int r = 0; r < nv; r++) {
    for (int c = 0; c < nv; c++) QT[(size_t)pad(c) * LD + pad(r)] = (float)Kinv[(size_t)r * NK + c];
    for (int m = 0; m < ne; m++) QbT[(size_t)m * LD + pad(r)] = (float)Kinv[(size_t)r * NK + nv + m];
  }
  auto* c = new mpcr_cem;
  c->device = device;
  c->nd = nd;
  c->H = H;
  c->max_n = max_n;
  if (hipMalloc(&c->d_X, sizeof(float) * X.size()) != hipSuccess ||
      hipMalloc(&c->d_QT, sizeof(float) * QT.size()) != hipSuccess ||
      hipMalloc(&c->d_QbT, sizeof(float) * QbT.size()) != hipSuccess ||
      hipMalloc(&c->d_LT, sizeof(float) * (size_t)LD * LD) != hipSuccess) {
    mpcr_cem_free(c);
    return fail(MPCR_ENOMEM, "device allocation failed");
  }
  if (hipMemcpy(c->d_X, X.data(), sizeof(float) * X.size(), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(c->d_QT, QT.data(), sizeof(float) * QT.size(), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(c->d_QbT, QbT.data(), sizeof(float) * QbT.size(), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemset(c->d_LT, 0, sizeof(float) * (size_t)LD * LD) != hipSuccess) {
    mpcr_cem_free(c);
    return fail(MPCR_EHIP, "table upload failed");
  }
  *out = c;
  return MPCR_OK;
}

extern "C" void mpcr_cem_free(mpcr_cem* c) {
  if (!c) return;
  (void)hipFree(c->d_X);
  (void)hipFree(c->d_QT);
  (void)hipFree(c->d_QbT);
  (void)hipFree(c->d_LT);
  delete c;
}

// mpcr_cem_factor (nprob = 1) and mpcr_cem_factor_multi: one workgroup per problem
static int cem_factor(mpcr_cem* c, const float* cov, int nprob, float reg, int flags, void* stream) {
  if (!c || !cov) return fail(MPCR_EINVAL, "null argument");
  if (!(flags & MPCR_F_DEVICE_PTRS)) return fail(MPCR_EINVAL, "mpcr_cem_factor takes device pointers");
  if (nprob < 1 || nprob > c->nprob)
    return fail(MPCR_EINVAL, "nprob=%d outside [1, %d] (mpcr_cem_set_problems)", nprob, c->nprob);
  HIPCHK(hipSetDevice(c->device));
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(cholesky_kernel, dim3(nprob), dim3(256), 0, st, cov, c->nd, reg, c->d_LT);
  HIPCHK(hipGetLastError());
  c->factored_n = nprob;
  if (flags & MPCR_F_SYNC) HIPCHK(hipStreamSynchronize(st));
  return MPCR_OK;
}

extern "C" int mpcr_cem_factor(mpcr_cem* c, const float* cov, float reg, int flags, void* stream) {
  return cem_factor(c, cov, 1, reg, flags, stream);
}

// Room for nprob Cholesky factors (the multi-problem entry points).  An
// explicit call, never lazy: a tick's launches stay graph-capturable.
extern "C" int mpcr_cem_set_problems(mpcr_cem* c, int nprob) {
  if (!c) return fail(MPCR_EINVAL, "null argument");
  if (nprob < 1 || nprob > c->max_n) return fail(MPCR_EINVAL, "nprob=%d outside [1, max_n=%d]", nprob, c->max_n);
  if (nprob == c->nprob) return MPCR_OK;
  HIPCHK(hipSetDevice(c->device));
  const size_t LD = (size_t)c->nd * PJ_BLK, bytes = sizeof(float) * LD * LD * nprob;
  float* lt = nullptr;
  HIPCHK(hipDeviceSynchronize());  // launches that still read the old factors
  if (hipMalloc(&lt, bytes) != hipSuccess) return fail(MPCR_ENOMEM, "device allocation failed");
  if (hipMemset(lt, 0, bytes) != hipSuccess) {
    (void)hipFree(lt);
    return fail(MPCR_EHIP, "factor storage initialisation failed");
  }
  (void)hipFree(c->d_LT);
  c->d_LT = lt;
  c->nprob = nprob;
  c->factored_n = 0;
  return MPCR_OK;
}

extern "C" int mpcr_cem_factor_multi(mpcr_cem* c, const float* cov, int nprob, float reg, int flags, void* stream) {
  return cem_factor(c, cov, nprob, reg, flags, stream);
}

// mpcr_cem_sample_project (nprob = 1, n candidates) and _multi (nprob
// problems of n candidates each): one launch, the problem on the grid's y
static int sample_project_launch(mpcr_cem* c, int nprob, int n, const float* mean, uint64_t seed, uint64_t seed_step,
                                 uint64_t counter, int index_base, const float* xi_in, float* xi_samples,
                                 const float* b_eq, int beq_stride, int beq_pstride, int maxiter, const float* bounds,
                                 float rho, float* xi_out, int flags, void* stream) {
  if (!xi_out) return fail(MPCR_EINVAL, "null argument");
  if (!(flags & MPCR_F_DEVICE_PTRS)) return fail(MPCR_EINVAL, "mpcr_cem_sample_project takes device pointers");
  if (!mean && !xi_in) return fail(MPCR_EINVAL, "need mean (sampling) or xi_in");
  if (mean && c->factored_n < nprob)
    return fail(MPCR_EINVAL, "sampling %d problem(s) after a factor call that covered %d (mpcr_cem_factor)", nprob,
                c->factored_n);
  if (maxiter < 0 || (maxiter > 0 && (!b_eq || !bounds || beq_stride < 0)))
    return fail(MPCR_EINVAL, "projection needs b_eq, bounds and maxiter >= 0");
  if (n == 0) return MPCR_OK;
  HIPCHK(hipSetDevice(c->device));
  hipStream_t st = (hipStream_t)stream;
  ProjArgs a;
  std::memset(&a, 0, sizeof(a));
  a.xi_in = xi_in;
  a.mean = mean;
  a.L = c->d_LT;
  a.xi_samples = xi_samples;
  a.beq = b_eq;
  a.xi_out = xi_out;
  a.X = c->d_X;
  a.QT = c->d_QT;
  a.QbT = c->d_QbT;
  a.seed = seed;
  a.counter = counter;
  a.index_base = index_base;
  a.n = n;
  a.nd = c->nd;
  a.H = c->H;
  a.maxiter = maxiter;
  a.beq_stride = beq_stride;
  a.seed_step = seed_step;
  a.beq_pstride = beq_pstride;
  for (int k = 0; k < 3; k++) a.bound[k] = bounds ? bounds[k] : 0.f;
  a.rho = rho;
  // the candidates' padded rows and the constraint rows X (3 x H x 12) in LDS;
  // a workgroup never straddles two problems (each has its own ragged tail)
  const int cpw = (long long)nprob * n >= PJ_CPW_SWITCH ? PJ_CPW_LARGE : PJ_CPW_SMALL;
  const size_t lds = sizeof(float) * (cpw * (c->nd * PJ_BLK + 4) + 3 * (size_t)c->H * PJ_BLK);
  const dim3 grid((n + cpw - 1) / cpw, nprob);
  if (cpw == PJ_CPW_LARGE)
    hipLaunchKernelGGL(sample_project_kernel<PJ_CPW_LARGE>, grid, dim3(64 * c->nd), lds, st, a);
  else
    hipLaunchKernelGGL(sample_project_kernel<PJ_CPW_SMALL>, grid, dim3(64 * c->nd), lds, st, a);
  HIPCHK(hipGetLastError());
  if (flags & MPCR_F_SYNC) HIPCHK(hipStreamSynchronize(st));
  return MPCR_OK;
}

extern "C" int mpcr_cem_sample_project(mpcr_cem* c, int n, const float* mean, uint64_t seed, uint64_t counter,
                                       int index_base, const float* xi_in, float* xi_samples, const float* b_eq, int beq_stride,
                                       int maxiter, const float* bounds, float rho, float* xi_out, int flags,
                                       void* stream) {
  if (!c) return fail(MPCR_EINVAL, "null argument");
  if (n < 0 || n > c->max_n) return fail(MPCR_EINVAL, "n=%d outside [0, max_n=%d]", n, c->max_n);
  return sample_project_launch(c, 1, n, mean, seed, 0, counter, index_base, xi_in, xi_samples, b_eq, beq_stride, 0,
                               maxiter, bounds, rho, xi_out, flags, stream);
}

// every candidate of problem p reads the boundary row b_eq + 5 nd p
extern "C" int mpcr_cem_sample_project_multi(mpcr_cem* c, int nprob, int n_per, const float* mean, uint64_t seed,
                                             uint64_t seed_step, uint64_t counter, int index_base, const float* xi_in,
                                             float* xi_samples, const float* b_eq, int maxiter, const float* bounds,
                                             float rho, float* xi_out, int flags, void* stream) {
  if (!c) return fail(MPCR_EINVAL, "null argument");
  if (int rc = check_multi(nprob, n_per, c->max_n)) return rc;
  if (nprob > 65535) return fail(MPCR_EINVAL, "nprob=%d exceeds the grid's 65535", nprob);
  return sample_project_launch(c, nprob, n_per, mean, seed, seed_step, counter, index_base, xi_in, xi_samples, b_eq, 0,
                               5 * c->nd, maxiter, bounds, rho, xi_out, flags, stream);
}

extern "C" int mpcr_project(mpcr_cem* c, const float* xi, const float* b_eq, int beq_stride, int n, int maxiter,
                            const float* bounds, float rho, float* xi_out, int flags, void* stream) {
  if (!xi) return fail(MPCR_EINVAL, "null xi");
  return mpcr_cem_sample_project(c, n, nullptr, 0, 0, 0, xi, nullptr, b_eq, beq_stride, maxiter, bounds, rho, xi_out,
                                 flags, stream);
}

// mpcr_cem_update (nprob = 1) and mpcr_cem_update_multi: one workgroup per problem
static int cem_update(mpcr_cem* c, const float* xi, int nprob, int n_per, const float* cost, int stride,
                      const int* elite_idx, int k, float lamda, float alpha_mean, float alpha_cov, float reg,
                      float* mean, float* cov, int flags, void* stream) {
  if (!c || !xi || !cost || !elite_idx || !mean || !cov || stride <= 0) return fail(MPCR_EINVAL, "null argument");
  if (!(flags & MPCR_F_DEVICE_PTRS)) return fail(MPCR_EINVAL, "mpcr_cem_update takes device pointers");
  if (k <= 0 || k > n_per || k > TOPK_MAX)
    return fail(MPCR_EINVAL, "k=%d outside [1, min(n=%d, %d)]", k, n_per, TOPK_MAX);
  HIPCHK(hipSetDevice(c->device));
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(cem_update_kernel, dim3(nprob), dim3(1024), 0, st, xi, n_per, c->nd * PJ_NB, cost, stride,
                     elite_idx, k, lamda, alpha_mean, alpha_cov, reg, mean, cov);
  HIPCHK(hipGetLastError());
  if (flags & MPCR_F_SYNC) HIPCHK(hipStreamSynchronize(st));
  return MPCR_OK;
}

extern "C" int mpcr_cem_update(mpcr_cem* c, const float* xi, int n, const float* cost, int stride,
                               const int* elite_idx, int k, float lamda, float alpha_mean, float alpha_cov, float reg,
                               float* mean, float* cov, int flags, void* stream) {
  return cem_update(c, xi, 1, n, cost, stride, elite_idx, k, lamda, alpha_mean, alpha_cov, reg, mean, cov, flags,
                    stream);
}

extern "C" int mpcr_cem_update_multi(mpcr_cem* c, const float* xi, int nprob, int n_per, const float* cost, int stride,
                                     const int* elite_idx, int k, float lamda, float alpha_mean, float alpha_cov,
                                     float reg, float* mean, float* cov, int flags, void* stream) {
  if (!c) return fail(MPCR_EINVAL, "null argument");
  if (int rc = check_multi(nprob, n_per, c->max_n)) return rc;
  return cem_update(c, xi, nprob, n_per, cost, stride, elite_idx, k, lamda, alpha_mean, alpha_cov, reg, mean, cov,
                    flags, stream);
}

#include "comm.hip"
