// api.cpp -- the extern "C" entry points of librtbhip.so (declared in include/rtbhip.h).
// Argument checking, handle registry, lazy per-device upload of the chain / link tables, and the
// host-memory convenience path (stage -> launch -> copy back).  No arithmetic lives here.
// Layout: the shared plumbing (errors, tracing, registry, uploads, staging, argument checks), then one body per entry FAMILY in an
// anonymous namespace, then the exported functions, which only name their family and pass their arguments on.
#include "rtbhip_internal.h"
#include "partial_device.h"
#include "frames_device.h"
#include "tree_device.h"
#include "kin_reg.h"
#include <atomic>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <dlfcn.h>
#include <map>
#include <memory>
#include <type_traits>
#include <unordered_map>
#include <functional>

namespace rtbhip {

// defined next to the kernels they serve; not in a header: every header of csrc/ is part of the run-time compiler's source digest
void kin_tune(const char *key, int value);
void rne_tune(const char *key, int value);
void ik_tune(const char *key, int value);
void partial_tune(const char *key, int value);
void hostpipe_tune(const char *key, int value);
void shard_tune(const char *key, int value);
void tree_tune(const char *key, int value);
void ik_release_device_state();
int ik_prepare_device();
std::string tree_jit_knowledge(const Tree *t, std::string *type_name);      // tree_kernels.hip
bool tree_jit_applies(const Tree *t);

// ---------------------------------------------------------------- errors
static thread_local std::string g_err;
static thread_local int g_last_launch[3] = {0, 0, 0};

void set_error(const std::string &msg) { g_err = msg; }
int hip_fail(hipError_t e, const char *what)
{
    g_err = std::string(what) + ": " + hipGetErrorString(e);
    (void)hipGetLastError();  // clear sticky state where possible
    return RTBHIP_EHIP;
}
void note_launch(int grid, int block, int lds)
{
    g_last_launch[0] = grid; g_last_launch[1] = block; g_last_launch[2] = lds;
}

// ---------------------------------------------------------------- tracing ranges (opt-in)
// RTBHIP_ROCTX=1: every compute entry point is bracketed by a roctx range named after it, so `rocprofv3 --marker-trace`
// shows which ABI call a kernel belongs to (the reference has no tracing hooks).  The marker library is looked
// up at run time -- nothing links against it and nothing happens when the variable is unset.
namespace {
struct Roctx {
    int (*push)(const char *) = nullptr;
    int (*pop)() = nullptr;
    Roctx()
    {
        const char *on = std::getenv("RTBHIP_ROCTX");
        if (!on || !*on || *on == '0') return;
        for (const char *name : {"librocprofiler-sdk-roctx.so.1", "librocprofiler-sdk-roctx.so", "libroctx64.so.4", "libroctx64.so"}) {
            if (void *h = dlopen(name, RTLD_NOW | RTLD_GLOBAL)) {
                push = (int (*)(const char *))dlsym(h, "roctxRangePushA");
                pop = (int (*)())dlsym(h, "roctxRangePop");
                if (push && pop) return;
                push = nullptr; pop = nullptr;
            }
        }
    }
};
const Roctx &roctx() { static const Roctx r; return r; }
struct TraceRange {       // named "rtbhip_" + fn; the name is only built when tracing is on
    bool on;
    explicit TraceRange(const char *fn) : on(roctx().push != nullptr) { if (on) roctx().push((std::string("rtbhip_") + fn).c_str()); }
    ~TraceRange() { if (on) roctx().pop(); }
    TraceRange(const TraceRange &) = delete;
};
}  // namespace
#define RTB_TRACE(fn) ::rtbhip::TraceRange _trace_range(fn)
#define RTB_TRY(expr)                   \
    do {                                \
        int _rc = (expr);               \
        if (_rc != RTBHIP_OK) return _rc; \
    } while (0)

// ---------------------------------------------------------------- handle registry
// The registries are heap objects that are never destroyed: handles that are still registered when the process exits (module-level
// robot objects whose Python __del__ never ran) must not have their destructors -- which call hipFree -- run during static
// destruction, possibly after the HIP runtime has been torn down.  The OS reclaims device memory with the process.
// One id counter serves all kinds, so a chain id is never a valid dyn or tree id.
static std::atomic<uint64_t> g_next{1};
namespace {
template <class T> struct Registry {
    std::mutex mu;
    std::unordered_map<uint64_t, std::shared_ptr<T>> map;
    uint64_t add(std::shared_ptr<T> obj)
    {
        const uint64_t h = g_next.fetch_add(1);
        std::lock_guard<std::mutex> lk(mu);
        map[h] = std::move(obj);
        return h;
    }
    std::shared_ptr<T> find(uint64_t h)
    {
        std::lock_guard<std::mutex> lk(mu);
        auto it = map.find(h);
        return it == map.end() ? nullptr : it->second;
    }
    std::shared_ptr<T> take(uint64_t h)          // the registry's reference leaves with the caller: the object goes with its last user
    {
        std::lock_guard<std::mutex> lk(mu);
        auto it = map.find(h);
        if (it == map.end()) return nullptr;
        std::shared_ptr<T> obj = std::move(it->second);
        map.erase(it);
        return obj;
    }
    int destroy(uint64_t h, const char *fn)
    {
        if (!take(h)) { set_error(std::string(fn) + ": unknown handle"); return RTBHIP_EINVAL; }
        return RTBHIP_OK;
    }
};
Registry<Chain> &g_chains = *new Registry<Chain>();
Registry<Dyn> &g_dyns = *new Registry<Dyn>();
Registry<Tree> &g_trees = *new Registry<Tree>();

// ---------------------------------------------------------------- per-device copies of a handle's tables
template <class P> void free_all(std::map<int, P *> &copies)
{
    for (auto &kv : copies) (void)hipFree(kv.second);
    copies.clear();
}
void drop_device_copies(Chain &c) { free_all(c.dev_ops); free_all(c.dev_qlim); }
void drop_device_copies(Dyn &d) { free_all(d.dev_links); }
void drop_device_copies(Tree &t) { free_all(t.dev_groups); }
// rtbhip_shutdown: handles stay valid, the tables are uploaded again on next use
template <class T> void drop_all_device_copies(Registry<T> &reg)
{
    std::lock_guard<std::mutex> lk(reg.mu);
    for (auto &kv : reg.map) {
        std::lock_guard<std::mutex> l2(kv.second->mu);
        drop_device_copies(*kv.second);
    }
}

// a device block of `alloc` bytes holding the first `bytes` of `host`; nothing stays allocated on failure
hipError_t upload_block(const void *host, size_t bytes, size_t alloc, void **out)
{
    void *p = nullptr;
    hipError_t e = hipMalloc(&p, alloc);
    if (e == hipSuccess && bytes) e = hipMemcpy(p, host, bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess && p) { (void)hipFree(p); p = nullptr; }
    *out = p;
    return e;
}
// an object's one table on the current device, uploaded on first use
template <class P> int device_table(std::mutex &mu, std::map<int, P *> &copies, const std::vector<P> &table, const char *what, const P **out)
{
    int dev = 0;
    RTB_HIP(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lk(mu);
    auto it = copies.find(dev);
    if (it == copies.end()) {
        void *p = nullptr;
        hipError_t e = upload_block(table.data(), table.size() * sizeof(P), table.size() * sizeof(P), &p);
        if (e != hipSuccess) return hip_fail(e, what);
        it = copies.emplace(dev, (P *)p).first;
    }
    *out = it->second;
    return RTBHIP_OK;
}
}  // namespace

std::shared_ptr<Chain> chain_from_handle(rtbhip_chain_t h) { return g_chains.find(h); }
std::shared_ptr<Dyn> dyn_from_handle(rtbhip_dyn_t h) { return g_dyns.find(h); }
std::shared_ptr<Tree> tree_from_handle(rtbhip_tree_t h) { return g_trees.find(h); }

Chain::~Chain() { drop_device_copies(*this); }
Dyn::~Dyn() { drop_device_copies(*this); }
Tree::~Tree() { drop_device_copies(*this); }

static DevChain view_of(const Chain *c, const void *base)
{
    DevChain v;
    const char *p = (const char *)base;
    v.seg = (const DevSeg *)p;
    p += c->seg.size() * sizeof(DevSeg);
    v.jmeta = (const int32_t *)p;
    return v;
}

DevChain chain_host_view(const Chain *c)
{
    DevChain v;
    v.seg = c->seg.data();
    v.jmeta = c->jmeta.data();
    return v;
}

int chain_device_ops(Chain *c, DevChain *out, const double **qlim_out)
{
    int dev = 0;
    RTB_HIP(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lk(c->mu);
    auto it = c->dev_ops.find(dev);
    if (it == c->dev_ops.end()) {
        std::vector<char> blob(c->seg.size() * sizeof(DevSeg) + c->jmeta.size() * sizeof(int32_t) + 16, 0);
        char *w = blob.data();
        std::memcpy(w, c->seg.data(), c->seg.size() * sizeof(DevSeg));
        w += c->seg.size() * sizeof(DevSeg);
        if (!c->jmeta.empty()) std::memcpy(w, c->jmeta.data(), c->jmeta.size() * sizeof(int32_t));
        void *d = nullptr, *ql = nullptr;
        hipError_t e = upload_block(blob.data(), blob.size(), blob.size(), &d);
        if (e == hipSuccess) e = upload_block(c->qlim.data(), c->qlim.size() * sizeof(double), (c->qlim.size() ? c->qlim.size() : 1) * sizeof(double), &ql);
        if (e != hipSuccess) {             // nothing half-uploaded stays behind
            if (d) (void)hipFree(d);
            return hip_fail(e, "chain table upload");
        }
        it = c->dev_ops.emplace(dev, d).first;
        c->dev_qlim[dev] = (double *)ql;
    }
    *out = view_of(c, it->second);
    if (qlim_out) *qlim_out = c->dev_qlim[dev];
    return RTBHIP_OK;
}

int dyn_device_links(Dyn *d, const DevLink **out) { return device_table(d->mu, d->dev_links, d->links, "link table upload", out); }
int tree_device_groups(Tree *t, const DevGroup **out) { return device_table(t->mu, t->dev_groups, t->groups, "tree table upload", out); }

// Stream-ordered temporaries (hipMallocAsync: the rows of the IK schedules, the lower-order tensors of partial_fkine0) come from the device's
// default memory pool.  Its release threshold is 0 by default: everything freed goes back to the OS at the next synchronisation, so EVERY
// call pays for fresh allocations (measured: 0.35 ms for the 99 MB of rows of a 1e5-target IK call).  Raised once per device: freed
// blocks stay in the pool; rtbhip_trim / rtbhip_shutdown hand them back.
int pool_keep_cached()
{
    static std::mutex mu;
    static std::map<int, bool> done;
    int dev = 0;
    RTB_HIP(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lk(mu);
    if (done[dev]) return RTBHIP_OK;
    hipMemPool_t pool;
    RTB_HIP(hipDeviceGetDefaultMemPool(&pool, dev));
    uint64_t keep = ~0ull;
    RTB_HIP(hipMemPoolSetAttribute(pool, hipMemPoolAttrReleaseThreshold, &keep));
    done[dev] = true;
    return RTBHIP_OK;
}

int device_cu_count(int *cus)
{
    int dev = 0;
    RTB_HIP(hipGetDevice(&dev));
    RTB_HIP(hipDeviceGetAttribute(cus, hipDeviceAttributeMultiprocessorCount, dev));
    return RTBHIP_OK;
}

namespace {

// ---------------------------------------------------------------- the staged host path
// The calls that are not row-pipelined (IK, the dynamics terms, the differential-kinematics consumers ...) name each buffer once, through
// in() / out(), and spell their launch once, on the pointers those return and on stream().  RTBHIP_MEM_DEVICE: the caller's own pointers and
// stream, finish() hands the launch's code back -- no HIP call, nothing allocated.  RTBHIP_MEM_HOST: device blocks from the cache of
// hostpipe.cpp (inputs uploaded), the NULL stream; finish() waits for the device and copies the outputs back in the order they were named.
// The high-volume calls -- fkine / jacob / fkine_jacob / hessian and rne -- go through host_pipeline instead.
class Staged {
    struct Buf { void *host, *dev; size_t bytes; };
    const bool host_;
    const hipStream_t stream_;
    int rc_ = RTBHIP_OK;
    std::vector<Buf> bufs_;               // host mode only; outputs have host != NULL

    int stage(const void *host, size_t bytes, void **dev, void *fetch_to)
    {
        RTB_TRY(dev_cache_alloc(bytes, dev));
        bufs_.push_back({fetch_to, *dev, bytes});
        if (host) RTB_HIP(hipMemcpy(*dev, host, bytes, hipMemcpyHostToDevice));
        return RTBHIP_OK;
    }
    void *add(const void *in_from, void *fetch_to, size_t bytes)
    {
        void *dev = nullptr;
        if (rc_ == RTBHIP_OK) rc_ = stage(in_from, bytes, &dev, fetch_to);
        return rc_ == RTBHIP_OK ? dev : nullptr;
    }
    int fetch_all()
    {
        RTB_HIP(hipDeviceSynchronize());
        for (const Buf &b : bufs_) {
            void *host = b.host;
            const void *dev = b.dev;
            const size_t bytes = b.bytes;
            if (host) RTB_HIP(hipMemcpy(host, dev, bytes, hipMemcpyDeviceToHost));
        }
        return RTBHIP_OK;
    }

public:
    Staged(int mem, void *stream) : host_(mem == RTBHIP_MEM_HOST), stream_(host_ ? nullptr : (hipStream_t)stream) {}
    ~Staged() { for (const Buf &b : bufs_) dev_cache_free(b.dev); }
    Staged(const Staged &) = delete;
    // the pointer the launcher reads / writes; host mode: NULL for a NULL array or zero bytes
    template <class T> const T *in(const T *p, size_t bytes) { return !host_ ? p : (p && bytes) ? (const T *)add(p, nullptr, bytes) : nullptr; }
    template <class T> T *out(T *p, size_t bytes) { return !host_ ? p : (p && bytes) ? (T *)add(nullptr, p, bytes) : nullptr; }
    hipStream_t stream() const { return stream_; }
    int status() const { return rc_; }    // of in() / out(): look at it before launching
    int finish(int launch_rc) { return (!host_ || launch_rc != RTBHIP_OK) ? launch_rc : fetch_all(); }
};

Affine affine_from16(const double *m16)
{
    Affine a;
    a.used = m16 != nullptr;
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 4; c++) a.v[4 * r + c] = m16 ? m16[4 * r + c] : (r == c ? 1.0 : 0.0);
    return a;
}

// ---------------------------------------------------------------- argument checks shared by the entry families
// The device a device-pointer call runs on.  The caller's buffers decide: when they live on a GPU other than the current one
// (a tensor on cuda:1 while device 0 is current -- a single process driving several GPUs) the call switches to that GPU for its
// duration -- table look-up / upload, launch geometry and the launch itself all happen there -- and the destructor restores the
// caller's current device.  `stream` must be a stream of the buffers' device (NULL = that device's default stream).
struct DeviceScope {
    int prev = -1;
    ~DeviceScope() { if (prev >= 0) (void)hipSetDevice(prev); }
    int enter_for(const char *fn, const void *buf)
    {
        hipPointerAttribute_t at;
        int cur = 0;
        if (buf && hipPointerGetAttributes(&at, buf) == hipSuccess && hipGetDevice(&cur) == hipSuccess) {
            if (at.type == hipMemoryTypeDevice && at.device != cur && prev < 0) {
                hipError_t e = hipSetDevice(at.device);
                if (e != hipSuccess) return hip_fail(e, (std::string(fn) + ": hipSetDevice to the buffer's GPU").c_str());
                prev = cur;
            }
        } else {
            (void)hipGetLastError();
        }
        return RTBHIP_OK;
    }
};

int refuse(const char *fn, const char *why, int rc = RTBHIP_EINVAL)
{
    set_error(std::string(fn) + ": " + why);
    return rc;
}

int check_mem(const char *fn, int mem)
{
    return mem != RTBHIP_MEM_HOST && mem != RTBHIP_MEM_DEVICE ? refuse(fn, "bad mem kind") : RTBHIP_OK;
}

int check_batch(const char *fn, const void *q, int64_t N, int mem, DeviceScope *scope)
{
    if (N < 0) return refuse(fn, "negative N");
    if (N > 0 && q == nullptr) return refuse(fn, "NULL input with N > 0");
    RTB_TRY(check_mem(fn, mem));
    if (mem == RTBHIP_MEM_DEVICE && N > 0 && scope) return scope->enter_for(fn, q);
    return RTBHIP_OK;
}

// float32 rows (rtbhip_fkine_jacob_f32, rtbhip_fkine_jacob_packed_f32, rtbhip_rne_f32) share the validation of the fp64 entries; host
// pointers are refused -- the host path converts nothing and is bound by the PCIe link, not by the width of a row (hostpipe.cpp is fp64 only)
template <class R> int check_row_type(const char *fn, int mem)
{
    if (std::is_same<R, float>::value && mem == RTBHIP_MEM_HOST) return refuse(fn, "float32 rows are served in device memory only (mem must be RTBHIP_MEM_DEVICE)");
    return RTBHIP_OK;
}

bool misaligned16(const void *a, const void *b, const void *c = nullptr) { return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & 15) != 0; }
constexpr const char *kAlign16 = "device buffers must be 16-byte aligned";

// ---------------------------------------------------------------- kinematics: fkine / jacob / hessian in any combination, or one packed [T | J] row
// fp64 rows: device pointers, or host arrays streamed through the two-slot pipeline (hostpipe.cpp) -- the same functor either way, applied to
// the caller's pointers or to device copies of one chunk
int kin_run(const Chain *c, const DevChain &ops, const double *q, int64_t N, const Affine &base, const Affine &tool, int frame, double *T, double *J,
            double *H, double *TJ, int mem, void *stream)
{
    const size_t n = (size_t)c->n;
    HostIO io;
    io.add_in(q, (size_t)c->q_width * 8);
    if (TJ) {
        io.add_out(TJ, 128 + 48 * n);
    } else {
        io.add_out(T, 128);
        io.add_out(J, 48 * n);
        io.add_out(H, 48 * n * n);
    }
    auto launch = [&](const void *const *din, void *const *dout, int64_t, int64_t rows, hipStream_t s) {
        if (TJ) return launch_kin_packed(c, ops, (const double *)din[0], rows, base, tool, frame, (double *)dout[0], s);
        return launch_kin(c, ops, (const double *)din[0], rows, base, tool, frame, (double *)dout[0], (double *)dout[1], (double *)dout[2], s);
    };
    if (mem == RTBHIP_MEM_DEVICE) return launch(io.in, io.out, 0, N, (hipStream_t)stream);
    return host_pipeline(io, N, launch);
}

int kin_run(const Chain *c, const DevChain &ops, const float *q, int64_t N, const Affine &base, const Affine &tool, int frame, float *T, float *J,
            float *, float *TJ, int, void *stream)
{
    if (TJ) return launch_kin_packed_f32(c, ops, q, N, base, tool, frame, TJ, (hipStream_t)stream);
    return launch_kin_f32(c, ops, q, N, base, tool, frame, T, J, (hipStream_t)stream);
}

template <class R>
int kin_entry(const char *fn, rtbhip_chain_t h, const R *q, int64_t N, const double *base16, const double *tool16, int frame, R *T, R *J, R *H, R *TJ,
              int mem, void *stream)
{
    const std::shared_ptr<Chain> c_owner = chain_from_handle(h);
    Chain *c = c_owner.get();
    RTB_TRACE(fn);
    if (!c) return refuse(fn, "unknown chain handle");
    DeviceScope dscope;
    RTB_TRY(check_batch(fn, q, N, mem, &dscope));
    RTB_TRY(check_row_type<R>(fn, mem));
    if (frame != 0 && frame != 1) return refuse(fn, "frame must be 0 (jacob0) or 1 (jacobe)");
    if (N > 0 && !T && !J && !H && !TJ) return refuse(fn, "no output buffer");
    if (N == 0) return RTBHIP_OK;
    if (c->n == 0) {                  // a chain of constants: J is (N, 6, 0) and H (N, 0, 6, 0) -- nothing to write (the reference returns empty
        J = nullptr; H = nullptr;     // arrays) -- and a packed row is the pose alone, (N, 16): what the plain fkine kernel writes
        if (TJ) { T = TJ; TJ = nullptr; }
        if (!T) return RTBHIP_OK;
    }
    DevChain ops;
    RTB_TRY(chain_device_ops(c, &ops, nullptr));
    return kin_run(c, ops, q, N, affine_from16(base16), affine_from16(tool16), frame, T, J, H, TJ, mem, stream);
}

}  // namespace
// the launchers of the vector-Jacobian products (kin_kernels.hip); declared here, not in rtbhip_internal.h: that header is part of the text
// handed to the run-time compiler, whose code-object keys these host-only declarations have no business changing
int launch_kin_vjp(const Chain *c, const DevChain &dc, const double *q, int64_t N, const Affine &base, const Affine &tool, const double *gT,
                   const double *gJ, double *gq, hipStream_t s);
int launch_kin_vjp_f32(const Chain *c, const DevChain &dc, const float *q, int64_t N, const Affine &base, const Affine &tool, const float *gT,
                       const float *gJ, float *gq, hipStream_t s);
int launch_vjp_from_jac(int n, const double *T, const double *J, const double *gT, const double *gJ, int64_t N, double *gq, hipStream_t s);
namespace {

// rtbhip_fkine_jacob_vjp / rtbhip_fkine_jacob_vjp_f32: the gradient of a loss on fkine and / or jacob0 with respect to q (kin_kernels.hip: k_kin_vjp)
template <class R>
int kin_vjp_entry(const char *fn, rtbhip_chain_t h, const R *q, int64_t N, const double *base16, const double *tool16, const R *gT, const R *gJ,
                  R *gq, int mem, void *stream)
{
    const std::shared_ptr<Chain> c_owner = chain_from_handle(h);
    Chain *c = c_owner.get();
    RTB_TRACE(fn);
    if (!c) return refuse(fn, "unknown chain handle");
    DeviceScope dscope;
    RTB_TRY(check_batch(fn, q, N, mem, &dscope));
    RTB_TRY(check_row_type<R>(fn, mem));
    if (N > 0 && !gq) return refuse(fn, "NULL gq");
    if (N > 0 && !gT && !gJ) return refuse(fn, "gT and gJ are both NULL: there is nothing to differentiate");
    if (c->n < 1) return refuse(fn, "chain has no joints");
    if (N == 0) return RTBHIP_OK;
    DevChain ops;
    RTB_TRY(chain_device_ops(c, &ops, nullptr));
    const size_t rows = (size_t)N, n = (size_t)c->n, qbytes = rows * c->q_width * sizeof(R);
    Staged st(mem, stream);
    const R *dq = st.in(q, qbytes), *dgT = st.in(gT, rows * 16 * sizeof(R)), *dgJ = st.in(gJ, rows * 6 * n * sizeof(R));
    R *dgq = st.out(gq, qbytes);
    RTB_TRY(st.status());
    const Affine base = affine_from16(base16), tool = affine_from16(tool16);
    if constexpr (std::is_same<R, float>::value) return st.finish(launch_kin_vjp_f32(c, ops, dq, N, base, tool, dgT, dgJ, dgq, st.stream()));
    else return st.finish(launch_kin_vjp(c, ops, dq, N, base, tool, dgT, dgJ, dgq, st.stream()));
}

/* Robot.manipulability(J=...) / Robot.jacobm(J=..., H=...) (robot/Robot.py:701-905, :1101-1235): pure functions of the supplied arrays */
int diff_from_jac_entry(const char *fn, int mode, const double *J, const double *H, int64_t N, int32_t n, int32_t axes, double *out,
                        int32_t mem, void *stream)
{
    if (n < 1 || n > 16) return refuse(fn, "n must be 1..16", RTBHIP_ELIMIT);
    if ((axes & 63) == 0) return refuse(fn, "empty axes mask");
    if (N > 0 && !out) return refuse(fn, "NULL output");
    DeviceScope dscope;
    RTB_TRY(check_batch(fn, J, N, mem, &dscope));
    if (N == 0) return RTBHIP_OK;
    if (mem == RTBHIP_MEM_DEVICE && misaligned16(J, H)) return refuse(fn, kAlign16);
    Staged st(mem, stream);
    const size_t jb = (size_t)N * 48 * n;
    const double *dJ = st.in(J, jb), *dH = st.in(H, jb * n);
    double *dout = st.out(out, (size_t)N * 8 * (mode == 0 ? 1 : n));
    RTB_TRY(st.status());
    return st.finish(launch_diff_from_jac(mode, n, dJ, dH, N, axes, dout, st.stream()));
}

/* fknm.Angle_Axis (core/fknm.cpp:112-162 -> _angle_axis core/ik.cpp:241-286) and tools/p_servo.py:46-117, batched with broadcasting: what they
   check alike.  *N = 0: an empty batch, nothing to do.  `gain_ok` sits where rtbhip_p_servo looks at its gain vector. */
int check_pose_pair(const char *fn, const void *Te, int64_t nTe, const void *Tep, int64_t nTep, bool gain_ok, const void *out, const void *out2,
                    int mem, DeviceScope *scope, int64_t *N)
{
    *N = 0;
    RTB_TRY(check_mem(fn, mem));
    if (nTe < 0 || nTep < 0) return refuse(fn, "negative count");
    if (!gain_ok) return refuse(fn, "NULL gain");
    if (nTe == 0 || nTep == 0) return RTBHIP_OK;
    const int64_t n = nTe > nTep ? nTe : nTep;
    if ((nTe != n && nTe != 1) || (nTep != n && nTep != 1)) return refuse(fn, "the pose counts must be equal, or one of them 1");
    if (!Te || !Tep || !out || !out2) return refuse(fn, "NULL buffer");
    if (mem == RTBHIP_MEM_DEVICE) {
        if (misaligned16(Te, Tep, out)) return refuse(fn, kAlign16);
        RTB_TRY(scope->enter_for(fn, out));
    }
    *N = n;
    return RTBHIP_OK;
}

// (rtbhip_p_servo_error reports under the name of rtbhip_angle_axis, whose body it shares)
int pose_error_entry(const double *Te, int64_t nTe, const double *Tep, int64_t nTep, int method, double *e, int32_t mem, void *stream)
{
    DeviceScope dscope;
    int64_t N;
    RTB_TRY(check_pose_pair("angle_axis", Te, nTe, Tep, nTep, true, e, e, mem, &dscope, &N));
    if (N == 0) return RTBHIP_OK;
    Staged st(mem, stream);
    const double *dA = st.in(Te, (size_t)nTe * 128), *dB = st.in(Tep, (size_t)nTep * 128);
    double *dE = st.out(e, (size_t)N * 48);
    RTB_TRY(st.status());
    return st.finish(launch_angle_axis(dA, nTe, dB, nTep, N, dE, st.stream(), method));
}

/* Robot.jacob0_dot / ETS.manipulability (yoshikawa) / ETS.jacobm */
int diff_entry(const char *fn, rtbhip_chain_t h, int mode, int axes, const double *q, const double *qd, int64_t N,
               const double *tool16, int frame, double *out, int mem, void *stream)
{
    const std::shared_ptr<Chain> c_owner = chain_from_handle(h);
    Chain *c = c_owner.get();
    RTB_TRACE(fn);
    if (!c) return refuse(fn, "unknown chain handle");
    DeviceScope dscope;
    RTB_TRY(check_batch(fn, q, N, mem, &dscope));
    if (frame != 0 && frame != 1) return refuse(fn, "frame must be 0 or 1");
    if (mode != 0 && mode != 3 && mode != 4 && (axes & 63) == 0) return refuse(fn, "empty axes mask");
    const bool needs_qd = mode == 0 || mode == 4;
    if (N > 0 && (!out || (needs_qd && !qd))) return refuse(fn, "NULL qd/output");
    if (N == 0) return RTBHIP_OK;
    DevChain ops;
    RTB_TRY(chain_device_ops(c, &ops, nullptr));
    const size_t n = (size_t)c->n, qbytes = (size_t)N * c->q_width * 8;
    Staged st(mem, stream);
    const double *dq = st.in(q, qbytes), *dqd = st.in(qd, needs_qd ? qbytes : 0);
    double *dout = st.out(out, (size_t)N * 8 * ((mode == 0 || mode == 3 || mode == 4) ? 6 * n : (mode == 1 ? 1 : n)));
    RTB_TRY(st.status());
    return st.finish(launch_kin_diff(c, ops, mode, axes, dq, dqd, N, affine_from16(tool16), frame, dout, st.stream()));
}

// restart-generator key of row 0 for the IK calls this thread makes from now on (rtbhip.h)
thread_local int64_t t_ik_target_base = 0;

// rtbhip_ik_lm / rtbhip_ik_lm_nullspace / rtbhip_ik_qp (method 5: kj travels in lambda)
int ik_entry(rtbhip_chain_t chain, const double *Tep, int64_t N, const double *q0,
             int32_t ilimit, int32_t slimit, double tol, int32_t reject_jl, const double *we6,
             double lambda, int32_t method, int32_t flavour, uint64_t seed,
             double kq, double km, double ps, const double *pi, double ks, double *q_out,
             int32_t *success, int32_t *iters, int32_t *searches, double *residual,
             int32_t mem, void *stream)
{
    const char *fn = "ik_lm";
    const std::shared_ptr<Chain> c_owner = chain_from_handle(chain);
    Chain *c = c_owner.get();
    RTB_TRACE(fn);
    if (!c) return refuse(fn, "unknown chain handle");
    DeviceScope dscope;
    RTB_TRY(check_batch(fn, Tep, N, mem, &dscope));
    if (flavour < 0 || flavour > 1) return refuse(fn, "flavour must be 0 (ik_LM) or 1 (ikine_LM)");
    if (ilimit < 1 || slimit < 1) return refuse(fn, "ilimit and slimit must be >= 1");
    if (c->n < 1) return refuse(fn, "chain has no joints");
    if (c->q_width != c->n) return refuse(fn, "chain must use jindex 0..n-1 (reference ik.cpp:34-37 assumes the same)");
    if (N > 0 && (!q_out || !success || !iters || !searches || !residual)) return refuse(fn, "NULL output");
    if (N == 0) return RTBHIP_OK;
    IkParams p;
    p.ilimit = ilimit; p.slimit = slimit; p.reject_jl = reject_jl ? 1 : 0; p.method = method;
    p.flavour = flavour; p.tol = tol; p.lambda = lambda; p.seed = seed;
    p.kq = kq; p.km = km; p.ps = ps; p.ks = ks; p.target0 = t_ik_target_base;
    for (int j = 0; j < RTBHIP_MAX_JOINTS; ++j) p.pi[j] = pi ? pi[j < c->n ? j : (c->n > 0 ? c->n - 1 : 0)] : 0.3;      // NULL: the reference's default
    if (kq > 0.0 && flavour != 1) return refuse(fn, "null-space terms belong to the Python solvers (flavour 1)");
    if (kq > 0.0)
        for (int j = 0; j < c->n && j < RTBHIP_MAX_JOINTS; ++j)
            if (ps == p.pi[j]) return refuse(fn, "ps must differ from pi");
    for (int i = 0; i < 6; i++) p.we[i] = we6 ? we6[i] : 1.0;
    RTB_TRY(ik_check_limits(c, p, N));                 // what the device build refuses, before the device is touched
    DevChain ops;
    const double *qlim = nullptr;
    RTB_TRY(chain_device_ops(c, &ops, &qlim));
    const size_t rows = (size_t)N, qbytes = rows * (size_t)c->n * 8;
    Staged st(mem, stream);
    const double *dTep = st.in(Tep, rows * 128), *dq0 = st.in(q0, qbytes);
    double *dq = st.out(q_out, qbytes);
    int32_t *ds = st.out(success, rows * 4), *di = st.out(iters, rows * 4), *dse = st.out(searches, rows * 4);
    double *dr = st.out(residual, rows * 8);
    RTB_TRY(st.status());
    return st.finish(launch_ik(c, ops, qlim, dTep, N, dq0, p, dq, ds, di, dse, dr, st.stream()));
}

// ---------------------------------------------------------------- dynamics
// rtbhip_rne / rtbhip_rne_base_wrench: device pointers or the host pipeline, one functor; rtbhip_rne_f32: device rows only, no base wrench
int rne_run(const Dyn *d, const DevLink *links, const double *q, const double *qd, const double *qdd, int64_t N, const double *grav3,
            const double *fext6, double *tau, double *wbase, bool want_wbase, int mem, void *stream)
{
    HostIO io;
    const size_t row = (size_t)d->n * 8;
    io.add_in(q, row); io.add_in(qd, row); io.add_in(qdd, row);          // qd / qdd may be NULL (= zeros): skipped, not staged
    io.add_out(tau, row);
    if (want_wbase) io.add_out(wbase, 6 * 8);
    auto launch = [&](const void *const *din, void *const *dout, int64_t, int64_t rows, hipStream_t s) {
        return launch_rne(d, links, (const double *)din[0], (const double *)din[1], (const double *)din[2], rows, grav3, fext6, (double *)dout[0], s,
                          want_wbase ? (double *)dout[1] : nullptr);
    };
    if (mem == RTBHIP_MEM_DEVICE) return launch(io.in, io.out, 0, N, (hipStream_t)stream);
    return host_pipeline(io, N, launch);
}

int rne_run(const Dyn *d, const DevLink *links, const float *q, const float *qd, const float *qdd, int64_t N, const double *grav3,
            const double *fext6, float *tau, float *, bool, int, void *stream)
{
    return launch_rne_f32(d, links, q, qd, qdd, N, grav3, fext6, tau, (hipStream_t)stream);
}

template <class R>
int rne_entry(const char *fn, rtbhip_dyn_t dyn, const R *q, const R *qd, const R *qdd, int64_t N, const double *grav3, const double *fext6, R *tau,
              R *wbase, bool want_wbase, int32_t mem, void *stream)
{
    RTB_TRACE(fn);
    const std::shared_ptr<Dyn> d_owner = dyn_from_handle(dyn);
    Dyn *d = d_owner.get();
    if (!d) return refuse(fn, "unknown dyn handle");
    DeviceScope dscope;
    RTB_TRY(check_batch(fn, q, N, mem, &dscope));
    RTB_TRY(check_row_type<R>(fn, mem));
    if (!grav3) return refuse(fn, "NULL gravity");
    if (N > 0 && !tau) return refuse(fn, "NULL tau");   // qd / qdd may be NULL (= zeros)
    if (want_wbase && N > 0 && !wbase) return refuse(fn, "NULL wbase");
    if (N == 0) return RTBHIP_OK;
    const DevLink *links = nullptr;
    RTB_TRY(dyn_device_links(d, &links));
    return rne_run(d, links, q, qd, qdd, N, grav3, fext6, tau, wbase, want_wbase, mem, stream);
}

}  // namespace
// the launchers of the inverse-dynamics adjoint (rne_vjp_kernels.hip); declared here for the reason launch_kin_vjp is, and WEAK: a library linked
// from this object without that unit (the CPU replay of the test suite) still loads, and refuses the two entry points
__attribute__((weak)) int launch_rne_vjp(const Dyn *d, const DevLink *links, const double *q, const double *qd, const double *qdd, int64_t N,
                                         const double *grav3, const double *fext6, const double *gtau, double *gq, double *gqd, double *gqdd,
                                         hipStream_t s);
__attribute__((weak)) int launch_rne_vjp_f32(const Dyn *d, const DevLink *links, const float *q, const float *qd, const float *qdd, int64_t N,
                                             const double *grav3, const double *fext6, const float *gtau, float *gq, float *gqd, float *gqdd,
                                             hipStream_t s);
// ... and of the link-tree adjoint (tree_rne_vjp_kernels.hip), weak for the same reason
__attribute__((weak)) int launch_tree_rne_vjp(const Tree *t, const DevGroup *groups, const double *q, const double *qd, const double *qdd, int64_t N,
                                              const double *grav3, const double *gtau, double *gq, double *gqd, double *gqdd, hipStream_t s);
// ... and of the all-frame adjoint of link_frames (frames_vjp_kernels.hip), weak for the same reason
__attribute__((weak)) int launch_frames_vjp(const Chain *c, const DevChain &dc, const FrameTable &ft, const double *q, int64_t N, const double *gF,
                                            double *gq, hipStream_t s);
// ... and of the two inertia-matrix adjoints (inertia_vjp_kernels.hip, tree_inertia_vjp_kernels.hip), weak for the same reason
__attribute__((weak)) int launch_inertia_vjp(const Dyn *d, const DevLink *links, const double *q, int64_t N, const double *gM, double *gq, hipStream_t s);
__attribute__((weak)) int launch_tree_inertia_vjp(const Tree *t, const DevGroup *groups, const double *q, int64_t N, const double *gM, double *gq,
                                                  hipStream_t s);
// ... and of the two Coriolis-matrix adjoints (coriolis_vjp_kernels.hip, tree_coriolis_vjp_kernels.hip), weak for the same reason
__attribute__((weak)) int launch_coriolis_vjp(const Dyn *d, const DevLink *links, const double *q, const double *qd, int64_t N, const double *gC,
                                              double *gq, double *gqd, hipStream_t s);
__attribute__((weak)) int launch_tree_coriolis_vjp(const Tree *t, const DevGroup *groups, const double *q, const double *qd, int64_t N,
                                                   const double *gC, double *gq, double *gqd, hipStream_t s);
// ... and of the implicit-function adjoint of the inverse kinematics (ikgrad_kernels.hip), weak for the same reason
__attribute__((weak)) int launch_ik_vjp(const Chain *c, const DevChain &dc, const double *q, int64_t N, const double *Tep, const int32_t *success,
                                        int rows, double d2, const double *gq, double *gTep, double *gtwist, hipStream_t s);
// ... and of resolved-rate motion control (rrmc_kernels.hip), weak for the same reason
__attribute__((weak)) int launch_rrmc(const Chain *c, const DevChain &dc, const rtbhip_rrmc_args *a, hipStream_t s);
// ... and of the reactive QP servo (mmc_kernels.hip), weak for the same reason
__attribute__((weak)) int launch_mmc(const Chain *c, const DevChain &dc, const rtbhip_mmc_args *a, hipStream_t s);
// ... and of the operational-space dynamics (opspace_kernels.hip, tree_opspace_kernels.hip), weak for the same reason
__attribute__((weak)) int launch_opspace(const Dyn *d, const DevLink *links, const double *q, const double *J, int64_t N, const double *grav3, int axes,
                                         double *Mx, double *Gx, double *asada, hipStream_t s);
__attribute__((weak)) int launch_tree_opspace(const Tree *t, const DevGroup *groups, const double *q, const double *J, int64_t N, const double *grav3,
                                              int axes, double *Mx, double *Gx, double *asada, hipStream_t s);
namespace {

/* the argument checks rtbhip_opspace and rtbhip_tree_opspace share (n: the robot's joints); RTBHIP_OK with *go = false: nothing to launch */
int opspace_check(const char *fn, int n, const double *q, const double *J, int64_t N, const double *grav3, int32_t axes_mask, const double *Mx,
                  const double *Gx, const double *asada, bool *go)
{
    *go = false;
    if (N < 0) return refuse(fn, "negative N");
    if (!Mx && !Gx && !asada) return refuse(fn, "Mx, Gx and asada are all NULL: there is nothing to compute");
    if (N > 0 && (!q || !J)) return refuse(fn, "NULL input with N > 0");
    if (Gx && !grav3) return refuse(fn, "NULL gravity with a Gx output");
    if (asada && (axes_mask & 63) == 0) return refuse(fn, "axes_mask selects no task-space row");
    if (n < 1 || n > 16) return refuse(fn, "robots of 1..16 joints", RTBHIP_ELIMIT);
    if (N == 0) return RTBHIP_OK;
    if ((N + 7) / 8 > 0x7fffffff) return refuse(fn, "batch too large for one launch", RTBHIP_ELIMIT);
    *go = true;
    return RTBHIP_OK;
}


// rtbhip_rne_vjp / rtbhip_rne_vjp_f32: the gradient of a loss on rtbhip_rne's torques with respect to q, qd and qdd (k_rne_vjp)
template <class R>
int rne_vjp_entry(const char *fn, rtbhip_dyn_t dyn, const R *q, const R *qd, const R *qdd, int64_t N, const double *grav3, const double *fext6,
                  const R *gtau, R *gq, R *gqd, R *gqdd, int32_t mem, void *stream)
{
    RTB_TRACE(fn);
    const std::shared_ptr<Dyn> d_owner = dyn_from_handle(dyn);
    Dyn *d = d_owner.get();
    if (!d) return refuse(fn, "unknown dyn handle");
    DeviceScope dscope;
    RTB_TRY(check_batch(fn, q, N, mem, &dscope));
    RTB_TRY(check_row_type<R>(fn, mem));
    if (N == 0) return RTBHIP_OK;                            // an empty batch: no pointer is looked at
    if (!gtau) return refuse(fn, "NULL gtau");               // qd / qdd may be NULL (= zeros)
    if (!gq && !gqd && !gqdd) return refuse(fn, "gq, gqd and gqdd are all NULL: there is nothing to compute");
    if (!grav3) return refuse(fn, "NULL gravity");           // (read on the host, as rtbhip_rne's)
    for (const DevLink &l : d->links)
        if (l.sigma != 0) return refuse(fn, "chain has a prismatic joint");
    const bool built = std::is_same<R, float>::value ? launch_rne_vjp_f32 != nullptr : launch_rne_vjp != nullptr;
    if (!built) return refuse(fn, "not built into this library");
    const DevLink *links = nullptr;
    RTB_TRY(dyn_device_links(d, &links));
    const size_t bytes = (size_t)N * (size_t)d->n * sizeof(R);
    Staged st(mem, stream);
    const R *dq = st.in(q, bytes), *dqd = st.in(qd, bytes), *dqdd = st.in(qdd, bytes), *dg = st.in(gtau, bytes);
    R *dgq = st.out(gq, bytes), *dgqd = st.out(gqd, bytes), *dgqdd = st.out(gqdd, bytes);
    RTB_TRY(st.status());
    if constexpr (std::is_same<R, float>::value) return st.finish(launch_rne_vjp_f32(d, links, dq, dqd, dqdd, N, grav3, fext6, dg, dgq, dgqd, dgqdd, st.stream()));
    else return st.finish(launch_rne_vjp(d, links, dq, dqd, dqdd, N, grav3, fext6, dg, dgq, dgqd, dgqdd, st.stream()));
}

/* Dynamics.inertia / coriolis / accel (robot/Dynamics.py:704-861, 424-509) of a DH arm (kind "dyn": dyn_from_handle, dyn_device_links,
   launch_dyn) and of an ETS robot's link tree over Robot.rne (kind "tree").  mode: 0 inertia, 1 coriolis, 2 accel. */
template <class Obj, class Table>
int dyn_terms_entry(const char *fn, const char *kind, const std::shared_ptr<Obj> owner, int (*table_of)(Obj *, const Table **),
                    int (*launch)(const Obj *, const Table *, int, const double *, const double *, const double *, int64_t, const double *, double *, hipStream_t),
                    int mode, const double *q, const double *qd, const double *tq, int64_t N, const double *grav3, double *out, int32_t mem, void *stream)
{
    Obj *d = owner.get();
    RTB_TRACE(fn);
    if (!d) return refuse(fn, (std::string("unknown ") + kind + " handle").c_str());
    DeviceScope dscope;
    RTB_TRY(check_batch(fn, q, N, mem, &dscope));
    if (N > 0 && !out) return refuse(fn, "NULL output");
    if (N > 0 && mode >= 1 && !qd) return refuse(fn, "NULL qd");
    if (N > 0 && mode == 2 && (!tq || !grav3)) return refuse(fn, "NULL torque/gravity");
    if (N == 0) return RTBHIP_OK;
    const Table *table = nullptr;
    RTB_TRY(table_of(d, &table));
    const size_t n = (size_t)d->n, bytes = (size_t)N * n * 8;
    Staged st(mem, stream);
    const double *dq = st.in(q, bytes), *dqd = st.in(qd, mode >= 1 ? bytes : 0), *dtq = st.in(tq, mode == 2 ? bytes : 0);
    double *dout = st.out(out, mode == 2 ? bytes : bytes * n);
    RTB_TRY(st.status());
    return st.finish(launch(d, table, mode, dq, dqd, dtq, N, grav3, dout, st.stream()));
}

int dyn_entry(const char *fn, rtbhip_dyn_t dyn, int mode, const double *q, const double *qd, const double *tq, int64_t N, const double *grav3,
              double *out, int32_t mem, void *stream)
{
    return dyn_terms_entry(fn, "dyn", dyn_from_handle(dyn), dyn_device_links, launch_dyn, mode, q, qd, tq, N, grav3, out, mem, stream);
}

int tree_dyn_entry(const char *fn, rtbhip_tree_t tree, int mode, const double *q, const double *qd, const double *tq, int64_t N, const double *grav3,
                   double *out, int32_t mem, void *stream)
{
    return dyn_terms_entry(fn, "tree", tree_from_handle(tree), tree_device_groups, launch_tree_dyn, mode, q, qd, tq, N, grav3, out, mem, stream);
}

// ---------------------------------------------------------------- a fleet: several chains, each with its own batch, one launch
int fleet_entry(const rtbhip_chain_t *chains, int32_t n_chains, const double *const *q,
                const int64_t *N, int32_t frame, double *const *T, double *const *J,
                int32_t mem, void *stream, bool packed)
{
    // packed: T[c] is the (N[c], 16 + 6 n_c) array of [T | J] rows, J is not used
    if (n_chains < 0 || (n_chains > 0 && (!chains || !q || !N || !T || (!packed && !J)))) { set_error("fleet: bad argument"); return RTBHIP_EINVAL; }
    RTB_TRACE(packed ? "fleet_fkine_jacob_packed" : "fleet_fkine_jacob");
    if (frame != 0 && frame != 1) return refuse("fleet", "frame must be 0 or 1");
    RTB_TRY(check_mem("fleet", mem));
    std::vector<FleetEntry> entries;
    Staged st(mem, stream);
    DeviceScope dscope;
    if (mem == RTBHIP_MEM_DEVICE)
        for (int i = 0; i < n_chains; i++)
            if (N[i] > 0 && q[i]) { RTB_TRY(dscope.enter_for("fleet", q[i])); break; }
    int64_t tile0 = 0;
    for (int i = 0; i < n_chains; i++) {
        const std::shared_ptr<Chain> c_owner = chain_from_handle(chains[i]);
        Chain *c = c_owner.get();
        if (!c) return refuse("fleet", "unknown chain handle");
        if (N[i] < 0) return refuse("fleet", "negative N");
        if (N[i] == 0) continue;
        if (!q[i] || !T[i] || (!packed && !J[i])) return refuse("fleet", "NULL buffer");
        FleetEntry e;
        RTB_TRY(chain_device_ops(c, &e.dc, nullptr));
        e.n = c->n; e.q_width = c->q_width; e.N = N[i]; e.tile0 = tile0;
        e.stride = 0; e.pad = 0;
        const size_t rows = (size_t)N[i], jbytes = rows * 48 * c->n;
        e.q = st.in(q[i], rows * c->q_width * 8);
        e.T = st.out(T[i], packed ? rows * 128 + jbytes : rows * 128);
        e.J = packed ? nullptr : st.out(J[i], jbytes);
        RTB_TRY(st.status());
        tile0 += (N[i] + 63) / 64;
        entries.push_back(e);
    }
    if (entries.empty()) return RTBHIP_OK;
    return st.finish(launch_fleet(entries, frame, st.stream(), packed));
}

// ask for a handle's run-time instantiations (jit.cpp).  At *_create: the kernels a first call is most likely to want; all = every variant.
void jit_request_chain(const Chain *c, bool touch)
{
    for (const std::string &e : ik_jit_names(c)) jit_request("ik_kernels.hip", e, std::string(), touch);
}
void jit_request_dyn(const Dyn *d, bool all, bool touch)
{
    const std::vector<std::string> nm = rne_jit_names(d);          // k_rne, k_rne_atrest, k_dyn x 3
    for (size_t i = 0; i < nm.size() && (all || i < 2); ++i) jit_request(i < 2 ? "rne_kernels.hip" : "dyn_kernels.hip", nm[i], std::string(), touch);
}
void jit_request_tree(const Tree *t, bool all, bool touch)
{
    const std::vector<std::string> nm = tree_jit_names(t);         // k_tree_rne (+ at rest), k_tree_dyn x 3
    if (nm.empty()) return;
    std::string tn;
    const std::string pre = tree_jit_knowledge(t, &tn);
    for (size_t i = 0; i < nm.size() && (all || i < 1); ++i)
        jit_request(nm[i].find("k_tree_dyn") != std::string::npos ? "tree_dyn_kernels.hip" : "tree_kernels.hip", nm[i], pre, touch);
}

// Make a handle's device table resident on `device` (-1: the current one) NOW: after this returns, device-pointer calls with the
// handle on that device only enqueue kernels -- no allocation, no synchronous copy -- so they can be captured into a hipGraph
// without a warm-up call.
int upload_on(int32_t device, const std::function<int()> &fn)
{
    int cur = 0;
    RTB_HIP(hipGetDevice(&cur));
    int have = 0;
    RTB_HIP(hipGetDeviceCount(&have));
    if (device < -1 || device >= have) { set_error("upload: no such device"); return RTBHIP_EINVAL; }
    const bool sw = device >= 0 && device != cur;
    if (sw) RTB_HIP(hipSetDevice(device));
    const int rc = fn();
    if (sw) (void)hipSetDevice(cur);
    return rc;
}

void trim_default_pool(size_t keep_bytes)      // the stream-ordered temporaries' pool (pool_keep_cached)
{
    int dev = 0;
    hipMemPool_t pool;
    if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetDefaultMemPool(&pool, dev) == hipSuccess) (void)hipMemPoolTrimTo(pool, keep_bytes);
    else (void)hipGetLastError();
}

int g_rne_pszero = 1;      // rtbhip_tune("rne_pszero", 0): handles created afterwards do not take the p* = 0 shortcut (A/B; same values)

}  // namespace
}  // namespace rtbhip

using namespace rtbhip;

extern "C" {

const char *rtbhip_last_error(void) { return g_err.c_str(); }
int rtbhip_version(void) { return 100; }

int rtbhip_init(int32_t n_devices)
{
    int have = 0;
    RTB_HIP(hipGetDeviceCount(&have));
    if (have < 1) { set_error("init: no HIP device is visible"); return RTBHIP_EHIP; }
    if (n_devices > have) { set_error("init: fewer HIP devices are visible than requested"); return RTBHIP_EHIP; }
    return RTBHIP_OK;
}

void rtbhip_shutdown(void)
{
    // device copies of every table are dropped (handles stay valid: tables are re-uploaded lazily on next use); one registry at a time, in this order
    drop_all_device_copies(g_chains);
    drop_all_device_copies(g_dyns);
    drop_all_device_copies(g_trees);
    ik_release_device_state();
    hostpipe_release();
    dev_cache_release();
    host_cache_trim(0);
    trim_default_pool(0);      // the stream-ordered temporaries of partial_fkine0 stay cached in the device's default pool: hand them back
}

int rtbhip_device_count(int *count)
{
    if (!count) { set_error("device_count: NULL"); return RTBHIP_EINVAL; }
    *count = 0;
    RTB_HIP(hipGetDeviceCount(count));
    return RTBHIP_OK;
}

// *_create: the handle's run-time instantiations are asked for (worker thread; nobody waits -- the first launches take the general kernels)
// BEFORE the registry is locked: the request computes signatures and may load the run-time compiler
int rtbhip_chain_create(const rtbhip_et *ets, int32_t m, const double *qlim, rtbhip_chain_t *chain)
{
    if (!chain) { set_error("chain_create: NULL out"); return RTBHIP_EINVAL; }
    std::shared_ptr<Chain> c(new Chain());
    RTB_TRY(compile_chain(ets, m, qlim, c.get()));
    jit_request_chain(c.get(), false);       // a chain without a built-in k_ik instantiation: its own
    *chain = g_chains.add(std::move(c));
    return RTBHIP_OK;
}

int rtbhip_chain_create_poe(const double *twists, int32_t n, const double *T0_16, const double *qlim, rtbhip_chain_t *chain)
{
    if (!chain) { set_error("chain_create_poe: NULL out"); return RTBHIP_EINVAL; }
    std::shared_ptr<Chain> c(new Chain());
    RTB_TRY(compile_poe(twists, n, T0_16, qlim, c.get()));
    jit_request_chain(c.get(), false);
    *chain = g_chains.add(std::move(c));
    return RTBHIP_OK;
}

// rtbhip_chain_upload also sizes the per-device scheduler state rtbhip_ik_lm needs
int rtbhip_chain_upload(rtbhip_chain_t chain, int32_t device)
{
    const std::shared_ptr<Chain> c = chain_from_handle(chain);
    if (!c) { set_error("chain_upload: unknown handle"); return RTBHIP_EINVAL; }
    return upload_on(device, [&]() -> int {
        DevChain ops;
        RTB_TRY(chain_device_ops(c.get(), &ops, nullptr));
        return ik_prepare_device();
    });
}

int rtbhip_dyn_upload(rtbhip_dyn_t dyn, int32_t device)
{
    const std::shared_ptr<Dyn> d = dyn_from_handle(dyn);
    if (!d) { set_error("dyn_upload: unknown handle"); return RTBHIP_EINVAL; }
    return upload_on(device, [&]() -> int { const DevLink *l; return dyn_device_links(d.get(), &l); });
}

int rtbhip_tree_upload(rtbhip_tree_t tree, int32_t device)
{
    const std::shared_ptr<Tree> t = tree_from_handle(tree);
    if (!t) { set_error("tree_upload: unknown handle"); return RTBHIP_EINVAL; }
    return upload_on(device, [&]() -> int { const DevGroup *g; return tree_device_groups(t.get(), &g); });
}

// Hand idle cached memory back: device staging blocks of the host-pointer calls above `keep_device_bytes`, pinned host blocks above
// `keep_pinned_bytes` (0, 0 = everything that is not in use).
int rtbhip_trim(uint64_t keep_device_bytes, uint64_t keep_pinned_bytes)
{
    dev_cache_trim((size_t)keep_device_bytes);
    host_cache_trim((size_t)keep_pinned_bytes);
    trim_default_pool((size_t)keep_device_bytes);
    return RTBHIP_OK;
}

// *_destroy: the device tables go with the last reference (a launch in flight keeps one)
int rtbhip_chain_destroy(rtbhip_chain_t chain) { return g_chains.destroy(chain, "chain_destroy"); }
int rtbhip_dyn_destroy(rtbhip_dyn_t dyn) { return g_dyns.destroy(dyn, "dyn_destroy"); }
int rtbhip_tree_destroy(rtbhip_tree_t tree) { return g_trees.destroy(tree, "tree_destroy"); }

int rtbhip_chain_info(rtbhip_chain_t chain, int32_t *n, int32_t *m, int32_t *q_width)
{
    const std::shared_ptr<Chain> c_owner = chain_from_handle(chain);
    Chain *c = c_owner.get();
    if (!c) { set_error("chain_info: unknown handle"); return RTBHIP_EINVAL; }
    if (n) *n = c->n;
    if (m) *m = (int32_t)c->ets.size();
    if (q_width) *q_width = c->q_width;
    return RTBHIP_OK;
}

int rtbhip_chain_set_q_width(rtbhip_chain_t chain, int32_t q_width)
{
    const std::shared_ptr<Chain> c_owner = chain_from_handle(chain);
    Chain *c = c_owner.get();
    if (!c) { set_error("chain_set_q_width: unknown handle"); return RTBHIP_EINVAL; }
    int need = 0;
    for (int j = 0; j < c->n; ++j) need = std::max(need, jm_jq(c->jmeta[j]) + 1);
    if (q_width < need || q_width > 256) {
        set_error("chain_set_q_width: width " + std::to_string(q_width) + " outside [" + std::to_string(need) + ", 256] for this chain");
        return RTBHIP_EINVAL;
    }
    c->q_width = q_width;     // the kernels take the row pitch of q from here; the chain tables do not depend on it
    return RTBHIP_OK;
}

int rtbhip_fkine(rtbhip_chain_t chain, const double *q, int64_t N, const double *base16,
                 const double *tool16, double *T, int32_t mem, void *stream)
{
    if (N > 0 && !T) { set_error("fkine: NULL T"); return RTBHIP_EINVAL; }
    return kin_entry<double>("fkine", chain, q, N, base16, tool16, 0, T, nullptr, nullptr, nullptr, mem, stream);
}

int rtbhip_jacob(rtbhip_chain_t chain, const double *q, int64_t N, const double *tool16,
                 int32_t frame, double *J, int32_t mem, void *stream)
{
    if (N > 0 && !J) { set_error("jacob: NULL J"); return RTBHIP_EINVAL; }
    return kin_entry<double>("jacob", chain, q, N, nullptr, tool16, frame, nullptr, J, nullptr, nullptr, mem, stream);
}

int rtbhip_fkine_jacob(rtbhip_chain_t chain, const double *q, int64_t N, const double *base16,
                       const double *tool16, int32_t frame, double *T, double *J, int32_t mem,
                       void *stream)
{
    if (N > 0 && (!T || !J)) { set_error("fkine_jacob: NULL T or J"); return RTBHIP_EINVAL; }
    return kin_entry<double>("fkine_jacob", chain, q, N, base16, tool16, frame, T, J, nullptr, nullptr, mem, stream);
}

int rtbhip_fkine_jacob_packed(rtbhip_chain_t chain, const double *q, int64_t N, const double *base16,
                              const double *tool16, int32_t frame, double *TJ, int32_t mem, void *stream)
{
    return kin_entry<double>("fkine_jacob_packed", chain, q, N, base16, tool16, frame, nullptr, nullptr, nullptr, TJ, mem, stream);
}

int rtbhip_fkine_jacob_f32(rtbhip_chain_t chain, const float *q, int64_t N, const double *base16,
                           const double *tool16, int32_t frame, float *T, float *J, int32_t mem,
                           void *stream)
{
    return kin_entry<float>("fkine_jacob_f32", chain, q, N, base16, tool16, frame, T, J, nullptr, nullptr, mem, stream);
}

int rtbhip_fkine_jacob_packed_f32(rtbhip_chain_t chain, const float *q, int64_t N, const double *base16,
                                  const double *tool16, int32_t frame, float *TJ, int32_t mem, void *stream)
{
    if (N > 0 && !TJ) { set_error("fkine_jacob_packed_f32: no output buffer"); return RTBHIP_EINVAL; }
    return kin_entry<float>("fkine_jacob_packed_f32", chain, q, N, base16, tool16, frame, nullptr, nullptr, nullptr, TJ, mem, stream);
}

int rtbhip_hessian(rtbhip_chain_t chain, const double *q, int64_t N, const double *tool16,
                   int32_t frame, double *H, int32_t mem, void *stream)
{
    if (N > 0 && !H) { set_error("hessian: NULL H"); return RTBHIP_EINVAL; }
    return kin_entry<double>("hessian", chain, q, N, nullptr, tool16, frame, nullptr, nullptr, H, nullptr, mem, stream);
}

/* ETS_hessian0 / ETS_hessiane with a supplied Jacobian (core/fknm.cpp:583-783 -> _ETS_hessian core/methods.cpp:16-32) */
int rtbhip_hessian_from_jacobian(const double *J, int64_t N, int32_t n, double *H, int32_t mem, void *stream)
{
    const char *fn = "hessian_from_jacobian";
    RTB_TRACE(fn);
    DeviceScope dscope;
    RTB_TRY(check_batch(fn, J, N, mem, &dscope));
    if (n < 1 || n > RTBHIP_MAX_JOINTS) return refuse(fn, "n must be 1..RTBHIP_MAX_JOINTS", RTBHIP_ELIMIT);
    if (N > 0 && !H) return refuse(fn, "NULL H");
    if (N == 0) return RTBHIP_OK;
    if (mem == RTBHIP_MEM_DEVICE && misaligned16(J, H)) return refuse(fn, kAlign16);
    Staged st(mem, stream);
    const size_t jb = (size_t)N * 48 * n;
    const double *dJ = st.in(J, jb);
    double *dH = st.out(H, jb * n);
    RTB_TRY(st.status());
    return st.finish(launch_hess_from_jac(n, dJ, N, dH, st.stream()));
}

/* the gradient of a loss on T = base * _ETS_fkine(q) * tool (core/methods.cpp:318-352) and J = _ETS_jacob0(q, tool) (:112-207) with respect to q */
int rtbhip_fkine_jacob_vjp(rtbhip_chain_t chain, const double *q, int64_t N, const double *base16, const double *tool16, const double *gT,
                           const double *gJ, double *gq, int32_t mem, void *stream)
{
    return kin_vjp_entry<double>("fkine_jacob_vjp", chain, q, N, base16, tool16, gT, gJ, gq, mem, stream);
}

int rtbhip_fkine_jacob_vjp_f32(rtbhip_chain_t chain, const float *q, int64_t N, const double *base16, const double *tool16, const float *gT,
                               const float *gJ, float *gq, int32_t mem, void *stream)
{
    return kin_vjp_entry<float>("fkine_jacob_vjp_f32", chain, q, N, base16, tool16, gT, gJ, gq, mem, stream);
}

/* ... from a supplied pose and Jacobian: d(column c of _ETS_jacob0)/dq_k is a cross product of columns k and c (_ETS_hessian, core/methods.cpp:16-32) */
int rtbhip_kin_vjp_from_jacobian(const double *T, const double *J, const double *gT, const double *gJ, int64_t N, int32_t n, double *gq,
                                 int32_t mem, void *stream)
{
    const char *fn = "kin_vjp_from_jacobian";
    RTB_TRACE(fn);
    DeviceScope dscope;
    RTB_TRY(check_batch(fn, J, N, mem, &dscope));
    if (n < 1 || n > RTBHIP_MAX_JOINTS) return refuse(fn, "n must be 1..RTBHIP_MAX_JOINTS", RTBHIP_ELIMIT);
    if (N > 0 && !gq) return refuse(fn, "NULL gq");
    if (N > 0 && !gT && !gJ) return refuse(fn, "gT and gJ are both NULL: there is nothing to differentiate");
    if (N > 0 && gT && !T) return refuse(fn, "gT needs T");
    if (N == 0) return RTBHIP_OK;
    Staged st(mem, stream);
    const size_t rows = (size_t)N, jb = rows * 48 * n;
    const double *dT = st.in(gT ? T : nullptr, rows * 128), *dJ = st.in(J, jb), *dgT = st.in(gT, rows * 128), *dgJ = st.in(gJ, jb);
    double *dgq = st.out(gq, rows * 8 * n);
    RTB_TRY(st.status());
    return st.finish(launch_vjp_from_jac(n, dT, dJ, dgT, dgJ, N, dgq, st.stream()));
}

int rtbhip_manipulability_from_jacobian(const double *J, int64_t N, int32_t n, int32_t axes_mask, int32_t method, double *m, int32_t mem, void *stream)
{
    RTB_TRACE("manipulability_from_jacobian");
    if (method < 0 || method > 2) { set_error("manipulability_from_jacobian: method must be 0 yoshikawa, 1 minsingular, 2 invcondition"); return RTBHIP_EINVAL; }
    return diff_from_jac_entry("manipulability_from_jacobian", 0, J, nullptr, N, n, (axes_mask & 63) | (method << 8), m, mem, stream);
}

int rtbhip_jacobm_from_jacobian(const double *J, const double *H, int64_t N, int32_t n, int32_t axes_mask, double *Jm, int32_t mem, void *stream)
{
    RTB_TRACE("jacobm_from_jacobian");
    return diff_from_jac_entry("jacobm_from_jacobian", H ? 2 : 1, J, H, N, n, axes_mask & 63, Jm, mem, stream);
}

int rtbhip_angle_axis(const double *Te, int64_t nTe, const double *Tep, int64_t nTep, double *e, int32_t mem, void *stream)
{
    RTB_TRACE("angle_axis");
    return pose_error_entry(Te, nTe, Tep, nTep, 0, e, mem, stream);
}

/* the error vector of tools/p_servo.py:46-117: method 0 "angle-axis" (= rtbhip_angle_axis), 1 "rpy" (the reference's default) */
int rtbhip_p_servo_error(const double *Te, int64_t nTe, const double *Tep, int64_t nTep, int32_t method, double *e, int32_t mem, void *stream)
{
    RTB_TRACE("p_servo_error");
    if (method != 0 && method != 1) { set_error("p_servo_error: method must be 0 angle-axis or 1 rpy"); return RTBHIP_EINVAL; }
    return pose_error_entry(Te, nTe, Tep, nTep, method, e, mem, stream);
}

/* tools/p_servo.py:46-117 whole: v = diag(gain) e and arrived = sum|e| < threshold in the launch that forms e */
int rtbhip_p_servo(const double *Te, int64_t nTe, const double *Tep, int64_t nTep, int32_t method, const double *gain6, double threshold, double *v,
                   uint8_t *arrived, int32_t mem, void *stream)
{
    const char *fn = "p_servo";
    RTB_TRACE(fn);
    if (method != 0 && method != 1) return refuse(fn, "method must be 0 angle-axis or 1 rpy");
    DeviceScope dscope;
    int64_t N;
    RTB_TRY(check_pose_pair(fn, Te, nTe, Tep, nTep, gain6 != nullptr, v, arrived, mem, &dscope, &N));
    if (N == 0) return RTBHIP_OK;
    Staged st(mem, stream);
    const double *dA = st.in(Te, (size_t)nTe * 128), *dB = st.in(Tep, (size_t)nTep * 128);
    double *dV = st.out(v, (size_t)N * 48);
    unsigned char *dF = st.out(arrived, (size_t)N);
    RTB_TRY(st.status());
    return st.finish(launch_p_servo(dA, nTe, dB, nTep, N, method, gain6, threshold, dV, dF, st.stream()));
}

int rtbhip_jacob_dot(rtbhip_chain_t chain, const double *q, const double *qd, int64_t N, const double *tool16,
                     int32_t frame, double *Jd, int32_t mem, void *stream)
{
    return diff_entry("jacob_dot", chain, 0, 63, q, qd, N, tool16, frame, Jd, mem, stream);
}

int rtbhip_jacob0_analytical(rtbhip_chain_t chain, const double *q, int64_t N, const double *tool16, int32_t representation,
                             double *Ja, int32_t mem, void *stream)
{
    if (representation < 0 || representation > 3) { set_error("jacob0_analytical: representation must be 0 rpy/xyz, 1 rpy/zyx, 2 eul, 3 exp"); return RTBHIP_EINVAL; }
    return diff_entry("jacob0_analytical", chain, 3, representation, q, nullptr, N, tool16, 0, Ja, mem, stream);
}

int rtbhip_jacob0_dot_analytical(rtbhip_chain_t chain, const double *q, const double *qd, int64_t N, const double *tool16,
                                 int32_t representation, double *Jd, int32_t mem, void *stream)
{
    if (representation < 0 || representation > 3) { set_error("jacob0_dot_analytical: representation must be 0 rpy/xyz, 1 rpy/zyx, 2 eul, 3 exp"); return RTBHIP_EINVAL; }
    return diff_entry("jacob0_dot_analytical", chain, 4, representation, q, qd, N, tool16, 0, Jd, mem, stream);
}

int rtbhip_manipulability(rtbhip_chain_t chain, const double *q, int64_t N, const double *tool16, int32_t axes_mask,
                          int32_t method, double *m, int32_t mem, void *stream)
{
    if (method < 0 || method > 2) { set_error("manipulability: method must be 0 yoshikawa, 1 minsingular, 2 invcondition"); return RTBHIP_EINVAL; }
    return diff_entry("manipulability", chain, 1, (axes_mask & 63) | (method << 8), q, nullptr, N, tool16, 0, m, mem, stream);
}

int rtbhip_jacobm(rtbhip_chain_t chain, const double *q, int64_t N, const double *tool16, int32_t axes_mask, double *Jm,
                  int32_t mem, void *stream)
{
    return diff_entry("jacobm", chain, 2, axes_mask, q, nullptr, N, tool16, 0, Jm, mem, stream);
}

/* DHRobot.fkine_all / Robot.fkine_all (robot/DHRobot.py:1012-1064, robot/Robot.py:638-698), batched */
int rtbhip_link_frames(rtbhip_chain_t chain, const double *q, int64_t N, const double *base16, const int32_t *marks,
                       int32_t nmarks, double *out, int32_t mem, void *stream)
{
    const char *fn = "link_frames";
    const std::shared_ptr<Chain> c_owner = chain_from_handle(chain);
    Chain *c = c_owner.get();
    RTB_TRACE(fn);
    if (!c) return refuse(fn, "unknown chain handle");
    RTB_TRY(check_mem(fn, mem));
    if (N < 0) return refuse(fn, "negative N");
    if (nmarks > 0 && !marks) return refuse(fn, "NULL marks");
    FrameTable ft;
    RTB_TRY(compile_frames(c, marks, nmarks, &ft));
    if (N == 0 || nmarks == 0) return RTBHIP_OK;
    if ((c->q_width > 0 && !q) || !out) return refuse(fn, "NULL q / output");
    Affine b = affine_from16(base16);
    ft.has_base = b.used;
    for (int i = 0; i < 12; i++) ft.base[i] = b.v[i];
    DevChain ops;
    RTB_TRY(chain_device_ops(c, &ops, nullptr));
    Staged st(mem, stream);
    const double *dq = st.in(q, (size_t)N * c->q_width * 8);
    double *dout = st.out(out, (size_t)N * nmarks * 128);
    RTB_TRY(st.status());
    return st.finish(launch_frames(c, ops, ft, dq, N, dout, st.stream()));
}

/* the gradient of a loss on rtbhip_link_frames' poses with respect to q (k_frames_vjp): every frame in one launch */
int rtbhip_link_frames_vjp(rtbhip_chain_t chain, const double *q, int64_t N, const double *base16, const int32_t *marks, int32_t nmarks,
                           const double *gF, double *gq, int32_t mem, void *stream)
{
    const char *fn = "link_frames_vjp";
    const std::shared_ptr<Chain> c_owner = chain_from_handle(chain);
    Chain *c = c_owner.get();
    RTB_TRACE(fn);
    if (!c) return refuse(fn, "unknown chain handle");
    RTB_TRY(check_mem(fn, mem));
    if (N < 0) return refuse(fn, "negative N");
    if (nmarks > 0 && !marks) return refuse(fn, "NULL marks");
    if (N > 0 && (!q || (nmarks > 0 && !gF))) return refuse(fn, "NULL input with N > 0");
    if (N > 0 && !gq) return refuse(fn, "NULL gq");
    if (c->n < 1) return refuse(fn, "chain has no joints");
    FrameTable ft;
    if (int rc = compile_frames(c, marks, nmarks, &ft)) {      // the lowering of rtbhip_link_frames, and its verdicts under this call's name
        if (g_err.compare(0, 13, "link_frames: ") == 0) g_err = std::string(fn) + g_err.substr(11);
        return rc;
    }
    if (N == 0) return RTBHIP_OK;
    DeviceScope dscope;
    if (mem == RTBHIP_MEM_DEVICE) RTB_TRY(dscope.enter_for(fn, q));
    const size_t qbytes = (size_t)N * c->q_width * 8;
    if (nmarks == 0) {                                         // no frame, no dependence on q: zeros
        if (mem == RTBHIP_MEM_HOST) std::memset(gq, 0, qbytes);
        else RTB_HIP(hipMemsetAsync(gq, 0, qbytes, (hipStream_t)stream));
        return RTBHIP_OK;
    }
    if (!launch_frames_vjp) return refuse(fn, "not built into this library");
    Staged st(mem, stream);
    Affine b = affine_from16(base16);
    ft.has_base = b.used;
    for (int i = 0; i < 12; i++) ft.base[i] = b.v[i];
    DevChain ops;
    RTB_TRY(chain_device_ops(c, &ops, nullptr));
    const double *dq = st.in(q, qbytes), *dgF = st.in(gF, (size_t)N * nmarks * 128);
    double *dgq = st.out(gq, qbytes);
    RTB_TRY(st.status());
    return st.finish(launch_frames_vjp(c, ops, ft, dq, N, dgF, dgq, st.stream()));
}

/* ETS.partial_fkine0 (robot/ETS.py:1821-2013): order >= 3; orders 1 and 2 are jacob0 / hessian0 */
int rtbhip_partial_fkine0(rtbhip_chain_t chain, const double *q, int64_t N, const double *tool16, int32_t order,
                          double *out, int32_t mem, void *stream)
{
    const char *fn = "partial_fkine0";
    const std::shared_ptr<Chain> c_owner = chain_from_handle(chain);
    Chain *c = c_owner.get();
    RTB_TRACE(fn);
    if (!c) return refuse(fn, "unknown chain handle");
    DeviceScope dscope;
    RTB_TRY(check_batch(fn, q, N, mem, &dscope));
    if (order < 3 || order > kPartialMaxOrder) return refuse(fn, ("order must be 3.." + std::to_string(kPartialMaxOrder)).c_str());
    if (c->n < 1) return refuse(fn, "chain has no joints");
    if (N > 0 && !out) return refuse(fn, "NULL output");
    if (N == 0) return RTBHIP_OK;
    const int n = c->n;
    // the kernels' 24-bit index arithmetic (partial_device.h) holds n^order columns and 6 n^(order-1) doubles of the largest lower tensor per
    // configuration: refused here, before the output (805 MB per configuration for 16 joints at order 6) is staged and the lower orders are
    // allocated and launched -- launch_partial keeps its own check
    if ((int64_t)partial_size(n, order) / 6 >= (1 << 24) || (int64_t)partial_size(n, order - 1) >= (1 << 24))
        return refuse(fn, "tensor too large (n^order must stay below 2^24)", RTBHIP_ELIMIT);
    DevChain ops;
    RTB_TRY(chain_device_ops(c, &ops, nullptr));
    Affine base = affine_from16(nullptr), tool = affine_from16(tool16);
    Staged st(mem, stream);
    const double *dq = st.in(q, (size_t)N * c->q_width * 8);
    double *dout = st.out(out, (size_t)N * (size_t)partial_size(n, order) * 8);
    RTB_TRY(st.status());
    const hipStream_t s = st.stream();
    // the lower-order tensors are stream-ordered temporaries from the device's memory pool (kept cached between
    // calls): the call only enqueues work, as every other device-pointer entry point does
    RTB_TRY(pool_keep_cached());
    double *lower[kPartialMaxOrder] = {nullptr};
    int rc = RTBHIP_OK;
    const bool skip_h = order == 3 && partial3_needs_no_hessian(n);       // k_partial3 forms the Hessians from the Jacobians it stages
    for (int a = 1; a < order && rc == RTBHIP_OK; ++a) {
        if (a == 2 && skip_h) continue;
        void *p = nullptr;
        hipError_t e = hipMallocAsync(&p, (size_t)N * (size_t)partial_size(n, a) * 8, s);
        if (e != hipSuccess) rc = hip_fail(e, "hipMallocAsync (partial_fkine0 temporaries)");
        lower[a - 1] = (double *)p;
    }
    // the two specialised launches (register-resident Jacobian, staged Hessian) beat the combined generic tile
    if (rc == RTBHIP_OK) rc = launch_kin(c, ops, dq, N, base, tool, 0, nullptr, lower[0], nullptr, s);
    if (rc == RTBHIP_OK && !skip_h) rc = launch_kin(c, ops, dq, N, base, tool, 0, nullptr, nullptr, lower[1], s);
    for (int a = 3; a <= order && rc == RTBHIP_OK; ++a)
        rc = launch_partial(n, a, lower, N, a == order ? dout : lower[a - 1], s);
    for (int a = 1; a < order; ++a)
        if (lower[a - 1]) (void)hipFreeAsync(lower[a - 1], s);
    return st.finish(rc);
}

int rtbhip_ik_lm(rtbhip_chain_t chain, const double *Tep, int64_t N, const double *q0,
                 int32_t ilimit, int32_t slimit, double tol, int32_t reject_jl, const double *we6,
                 double lambda, int32_t method, int32_t flavour, uint64_t seed, double *q_out,
                 int32_t *success, int32_t *iters, int32_t *searches, double *residual,
                 int32_t mem, void *stream)
{
    return rtbhip_ik_lm_nullspace(chain, Tep, N, q0, ilimit, slimit, tol, reject_jl, we6, lambda, method, flavour, seed,
                                  0.0, 0.0, 0.1, nullptr, q_out, success, iters, searches, residual, mem, stream);
}

int rtbhip_ik_target_base(int64_t base)
{
    if (base < 0) { set_error("ik_target_base: negative base"); return RTBHIP_EINVAL; }
    t_ik_target_base = base;
    return RTBHIP_OK;
}

int rtbhip_ik_lm_nullspace(rtbhip_chain_t chain, const double *Tep, int64_t N, const double *q0,
                           int32_t ilimit, int32_t slimit, double tol, int32_t reject_jl, const double *we6,
                           double lambda, int32_t method, int32_t flavour, uint64_t seed,
                           double kq, double km, double ps, const double *pi, double *q_out,
                           int32_t *success, int32_t *iters, int32_t *searches, double *residual,
                           int32_t mem, void *stream)
{
    if (method < 0 || method > 4) { set_error("ik_lm: method must be 0 chan, 1 wampler, 2 sugihara, 3 gauss-newton, 4 newton-raphson"); return RTBHIP_EINVAL; }
    return ik_entry(chain, Tep, N, q0, ilimit, slimit, tol, reject_jl, we6, lambda, method, flavour, seed, kq, km, ps, pi, 1.0, q_out, success, iters,
                    searches, residual, mem, stream);
}

int rtbhip_ik_qp(rtbhip_chain_t chain, const double *Tep, int64_t N, const double *q0, int32_t ilimit, int32_t slimit, double tol,
                 int32_t reject_jl, const double *we6, uint64_t seed, double kj, double ks, double kq, double km, double ps, const double *pi,
                 double *q_out, int32_t *success, int32_t *iters, int32_t *searches, double *residual, int32_t mem, void *stream)
{
    if (!(kj > 0.0) || !(ks > 0.0)) { set_error("ik_qp: kj and ks must be positive (Q must be positive definite)"); return RTBHIP_EINVAL; }
    return ik_entry(chain, Tep, N, q0, ilimit, slimit, tol, reject_jl, we6, kj, 5, 1, seed, kq, km, ps, pi, ks, q_out, success, iters, searches,
                    residual, mem, stream);
}

/* the gradient of a loss on rtbhip_ik_lm's q with respect to the targets (k_ik_vjp): device pointers only, a backward pass sees nothing else */
int rtbhip_ik_vjp(rtbhip_chain_t chain, const double *q, int64_t N, const double *Tep, const int32_t *success, const double *we6, double damping,
                  const double *gq, double *gTep, double *gtwist, void *stream)
{
    const char *fn = "ik_vjp";
    const std::shared_ptr<Chain> c_owner = chain_from_handle(chain);
    Chain *c = c_owner.get();
    RTB_TRACE(fn);
    if (!c) return refuse(fn, "unknown chain handle");
    if (N < 0) return refuse(fn, "negative N");
    if (N > 0 && (!q || !Tep || !gq)) return refuse(fn, "NULL input with N > 0");
    if (N > 0 && !gTep && !gtwist) return refuse(fn, "gTep and gtwist are both NULL: there is nothing to compute");
    if (c->n < 1) return refuse(fn, "chain has no joints");
    if (c->q_width != c->n) return refuse(fn, "chain must use jindex 0..n-1 (as rtbhip_ik_lm, whose q_out this reads)");
    int rows = 0, used = 0;
    for (int r = 0; r < 6; ++r)
        if (!we6 || we6[r] != 0.0) { rows |= 1 << r; ++used; }
    if (used > c->n) return refuse(fn, "more used rows than joints: the solver's step is the least-squares one there, not differentiated here");
    if (!(damping >= 0.0) || !std::isfinite(damping)) return refuse(fn, "damping must be finite and >= 0");
    if (N == 0) return RTBHIP_OK;
    if ((N + 63) / 64 > 0x7fffffff) return refuse(fn, "batch too large for one launch", RTBHIP_ELIMIT);
    if (!launch_ik_vjp) return refuse(fn, "not built into this library");
    DeviceScope dscope;
    RTB_TRY(dscope.enter_for(fn, q));
    DevChain ops;
    RTB_TRY(chain_device_ops(c, &ops, nullptr));
    return launch_ik_vjp(c, ops, q, N, Tep, success, rows, damping * damping, gq, gTep, gtwist, (hipStream_t)stream);
}

/* resolved-rate motion control, one step or the servo loop on the device (k_rrmc): device pointers only, one parameter block */
int rtbhip_rrmc(const rtbhip_rrmc_args *a)
{
    const char *fn = "rrmc";
    RTB_TRACE(fn);
    if (!a) return refuse(fn, "NULL parameter block");
    if (a->size != sizeof(rtbhip_rrmc_args)) return refuse(fn, "size is not sizeof(rtbhip_rrmc_args): built against another header");
    const std::shared_ptr<Chain> c_owner = chain_from_handle(a->chain);
    Chain *c = c_owner.get();
    if (!c) return refuse(fn, "unknown chain handle");
    if (a->N < 0) return refuse(fn, "negative N");
    if (a->nTep != a->N && a->nTep != 1) return refuse(fn, "nTep must be N or 1");
    if (a->N > 0 && (!a->q || !a->Tep)) return refuse(fn, "NULL input with N > 0");
    if (a->N > 0 && !a->qd && !a->q_out) return refuse(fn, "qd and q_out are both NULL: there is nothing to compute");
    if (c->n < 1) return refuse(fn, "chain has no joints");
    if (c->q_width != c->n) return refuse(fn, "chain must use jindex 0..n-1");
    if (a->method != 0 && a->method != 1) return refuse(fn, "method must be 0 angle-axis or 1 rpy");
    if (!(a->damping >= 0.0) || !std::isfinite(a->damping)) return refuse(fn, "damping must be finite and >= 0");
    bool finite = std::isfinite(a->threshold) && std::isfinite(a->dt);
    for (int k = 0; k < 6; ++k) finite = finite && std::isfinite(a->gain6[k]);
    if (!finite) return refuse(fn, "gain6, threshold and dt must be finite");
    if (a->steps < 1) return refuse(fn, "steps must be at least 1");
    if (c->n > kKinRegMax) return refuse(fn, "chains of 1..10 joints", RTBHIP_ELIMIT);
    if (a->steps > 4096) return refuse(fn, "at most 4096 steps", RTBHIP_ELIMIT);
    if ((a->N + 63) / 64 > 0x7fffffff) return refuse(fn, "batch too large for one launch", RTBHIP_ELIMIT);
    if (a->N == 0) return RTBHIP_OK;
    if (!launch_rrmc) return refuse(fn, "not built into this library");
    DeviceScope dscope;
    RTB_TRY(dscope.enter_for(fn, a->q));
    DevChain ops;
    RTB_TRY(chain_device_ops(c, &ops, nullptr));
    return launch_rrmc(c, ops, a, (hipStream_t)a->stream);
}

/* the reactive QP servo, one step or the loop on the device (k_mmc): one parameter block; q, Tep and the outputs on the device, qlim / qdlim on the host */
int rtbhip_mmc(const rtbhip_mmc_args *a)
{
    const char *fn = "mmc";
    RTB_TRACE(fn);
    if (!a) return refuse(fn, "NULL parameter block");
    if (a->size != sizeof(rtbhip_mmc_args)) return refuse(fn, "size is not sizeof(rtbhip_mmc_args): built against another header");
    const std::shared_ptr<Chain> c_owner = chain_from_handle(a->chain);
    Chain *c = c_owner.get();
    if (!c) return refuse(fn, "unknown chain handle");
    if (a->N < 0) return refuse(fn, "negative N");
    if (a->nTep != a->N && a->nTep != 1) return refuse(fn, "nTep must be N or 1");
    if (a->N > 0 && (!a->q || !a->Tep || !a->qlim)) return refuse(fn, "NULL input with N > 0");
    if (a->N > 0 && !a->qd && !a->q_out) return refuse(fn, "qd and q_out are both NULL: there is nothing to compute");
    if (c->q_width != c->n) return refuse(fn, "chain must use jindex 0..n-1");
    if (a->method != 0 && a->method != 1) return refuse(fn, "method must be 0 angle-axis or 1 rpy");
    bool finite = std::isfinite(a->threshold) && std::isfinite(a->dt) && std::isfinite(a->Y) && std::isfinite(a->ks) && std::isfinite(a->km) &&
                  std::isfinite(a->ps) && std::isfinite(a->pi) && std::isfinite(a->damper_gain);
    for (int k = 0; k < 6; ++k) finite = finite && std::isfinite(a->gain6[k]);
    if (!finite) return refuse(fn, "gain6, threshold, dt, Y, ks, km, ps, pi and damper_gain must be finite");
    if (!(a->Y > 0.0) || !(a->ks > 0.0)) return refuse(fn, "Y and ks must be positive (the QP must be strictly convex)");
    if (a->km < 0.0) return refuse(fn, "km must be >= 0");
    if (a->ps < 0.0) return refuse(fn, "ps must be >= 0");
    if (!(a->pi > a->ps)) return refuse(fn, "pi must be above ps");
    if (a->steps < 1) return refuse(fn, "steps must be at least 1");
    if (c->n < 6 || c->n > kKinRegMax) return refuse(fn, "chains of 6..10 joints", RTBHIP_ELIMIT);
    if (a->steps > 4096) return refuse(fn, "at most 4096 steps", RTBHIP_ELIMIT);
    if (a->N / 64 + (a->N % 64 != 0) > 0x7fffffff) return refuse(fn, "batch too large for one launch", RTBHIP_ELIMIT);   // (no N + 63: it overflows)
    if (a->N == 0) return RTBHIP_OK;
    for (int j = 0; j < c->n; ++j) {             // host arrays, read now (and once more by the launcher, into the launch's parameters)
        if (std::isnan(a->qlim[j]) || std::isnan(a->qlim[c->n + j]) || (a->qdlim && std::isnan(a->qdlim[j]))) return refuse(fn, "NaN in qlim or qdlim");
        if (a->qdlim && a->qdlim[j] < 0.0) return refuse(fn, "qdlim must be >= 0");
    }
    if (!launch_mmc) return refuse(fn, "not built into this library");
    DeviceScope dscope;
    RTB_TRY(dscope.enter_for(fn, a->q));
    DevChain ops;
    RTB_TRY(chain_device_ops(c, &ops, nullptr));
    return launch_mmc(c, ops, a, (hipStream_t)a->stream);
}

int rtbhip_ik_restart(rtbhip_chain_t chain, uint64_t seed, int64_t target, int32_t search, double *q_n)
{
    const std::shared_ptr<Chain> c_owner = chain_from_handle(chain);
    Chain *c = c_owner.get();
    if (!c || !q_n) { set_error("ik_restart: bad argument"); return RTBHIP_EINVAL; }
    ik_restart_host(c, seed, target, search, q_n);
    return RTBHIP_OK;
}

int rtbhip_dyn_create(const double *L24, int32_t n, int32_t mdh, rtbhip_dyn_t *dyn)
{
    if (!L24 || !dyn || n < 1) { set_error("dyn_create: bad argument"); return RTBHIP_EINVAL; }
    if (n > RTBHIP_MAX_JOINTS) { set_error("dyn_create: more than RTBHIP_MAX_JOINTS links"); return RTBHIP_ELIMIT; }
    if (mdh != 0 && mdh != 1) { set_error("dyn_create: mdh must be 0 or 1"); return RTBHIP_EINVAL; }
    std::shared_ptr<Dyn> d(new Dyn());
    d->n = n;
    d->mdh = mdh;
    d->links.resize(n);
    for (int i = 0; i < n; i++) {
        const double *l = L24 + 24 * i;  // layout: DHRobot.py:1342-1358
        DevLink &k = d->links[i];
        std::memset(&k, 0, sizeof k);
        int sigma = (int)l[4];  // frne.c:279 casts the double to the enum the same way
        if (sigma != 0 && sigma != 1) { set_error("dyn_create: sigma must be 0 (R) or 1 (P)"); return RTBHIP_EINVAL; }
        k.sa = sin(l[0]); k.ca = cos(l[0]);  // frne.c:325-326 evaluates these per call; constant per link
        k.a = l[1]; k.theta = l[2]; k.d = l[3]; k.sigma = sigma; k.offset = l[5];
        k.m = l[6]; k.rx = l[7]; k.ry = l[8]; k.rz = l[9];
        for (int j = 0; j < 9; j++) k.I[j] = l[10 + j];
        k.Jm = l[19]; k.G = l[20]; k.B = l[21]; k.Tc0 = l[22]; k.Tc1 = l[23];
        k.gjm = k.G * k.G * k.Jm; k.gb = k.G * k.G * k.B; k.ag = fabs(k.G);
        k.flags = 0;
        if (k.rx == 0.0 && k.ry == 0.0 && k.rz == 0.0) k.flags |= kLinkRZero;
        if (k.I[1] == 0.0 && k.I[2] == 0.0 && k.I[3] == 0.0 && k.I[5] == 0.0 && k.I[6] == 0.0 && k.I[7] == 0.0) k.flags |= kLinkIDiag;
        if (g_rne_pszero && k.sigma == 0 && k.a == 0.0 && k.d == 0.0) k.flags |= kLinkPsZero;      // p* = 0 (DH Panda links 2 and 6, Puma560 link 5 and 6)
    }
    jit_request_dyn(d.get(), false, false);       // a table without a built-in instantiation: its own
    *dyn = g_dyns.add(std::move(d));
    return RTBHIP_OK;
}

int rtbhip_rne(rtbhip_dyn_t dyn, const double *q, const double *qd, const double *qdd, int64_t N,
               const double *grav3, const double *fext6, double *tau, int32_t mem, void *stream)
{
    return rne_entry<double>("rne", dyn, q, qd, qdd, N, grav3, fext6, tau, nullptr, false, mem, stream);
}

int rtbhip_rne_f32(rtbhip_dyn_t dyn, const float *q, const float *qd, const float *qdd, int64_t N,
                   const double *grav3, const double *fext6, float *tau, int32_t mem, void *stream)
{
    return rne_entry<float>("rne_f32", dyn, q, qd, qdd, N, grav3, fext6, tau, nullptr, false, mem, stream);
}

int rtbhip_rne_base_wrench(rtbhip_dyn_t dyn, const double *q, const double *qd, const double *qdd, int64_t N,
                           const double *grav3, const double *fext6, double *tau, double *wbase, int32_t mem, void *stream)
{
    return rne_entry<double>("rne_base_wrench", dyn, q, qd, qdd, N, grav3, fext6, tau, wbase, true, mem, stream);
}

int rtbhip_rne_vjp(rtbhip_dyn_t dyn, const double *q, const double *qd, const double *qdd, int64_t N, const double *grav3, const double *fext6,
                   const double *gtau, double *gq, double *gqd, double *gqdd, int32_t mem, void *stream)
{
    return rne_vjp_entry<double>("rne_vjp", dyn, q, qd, qdd, N, grav3, fext6, gtau, gq, gqd, gqdd, mem, stream);
}

int rtbhip_rne_vjp_f32(rtbhip_dyn_t dyn, const float *q, const float *qd, const float *qdd, int64_t N, const double *grav3, const double *fext6,
                       const float *gtau, float *gq, float *gqd, float *gqdd, int32_t mem, void *stream)
{
    return rne_vjp_entry<float>("rne_vjp_f32", dyn, q, qd, qdd, N, grav3, fext6, gtau, gq, gqd, gqdd, mem, stream);
}

int rtbhip_tree_create(const rtbhip_tree_group *groups, int32_t ng, rtbhip_tree_t *tree)
{
    if (!tree) { set_error("tree_create: NULL handle pointer"); return RTBHIP_EINVAL; }
    std::shared_ptr<Tree> t(new Tree());
    RTB_TRY(compile_tree(groups, ng, t.get()));
    jit_request_tree(t.get(), false, false);
    *tree = g_trees.add(std::move(t));
    return RTBHIP_OK;
}

int rtbhip_tree_rne(rtbhip_tree_t tree, const double *q, const double *qd, const double *qdd, int64_t N,
                    const double *gravity3, double *tau, int32_t mem, void *stream)
{
    const char *fn = "tree_rne";
    const std::shared_ptr<Tree> t_owner = tree_from_handle(tree);
    Tree *t = t_owner.get();
    RTB_TRACE(fn);
    if (!t) return refuse(fn, "unknown tree handle");
    DeviceScope dscope;
    RTB_TRY(check_batch(fn, q, N, mem, &dscope));
    if (!gravity3) return refuse(fn, "NULL gravity");
    if (N > 0 && !tau) return refuse(fn, "NULL tau");
    if (N == 0) return RTBHIP_OK;
    const DevGroup *groups = nullptr;
    RTB_TRY(tree_device_groups(t, &groups));
    Staged st(mem, stream);
    const size_t bytes = (size_t)N * t->n * 8;
    const double *dq = st.in(q, bytes), *dqd = st.in(qd, bytes), *dqdd = st.in(qdd, bytes);
    double *dtau = st.out(tau, bytes);
    RTB_TRY(st.status());
    return st.finish(launch_tree_rne(t, groups, dq, dqd, dqdd, N, gravity3, dtau, st.stream()));
}

// the gradient of a loss on rtbhip_tree_rne's torques with respect to q, qd and qdd (k_tree_rne_vjp)
int rtbhip_tree_rne_vjp(rtbhip_tree_t tree, const double *q, const double *qd, const double *qdd, int64_t N, const double *gravity3,
                        const double *gtau, double *gq, double *gqd, double *gqdd, int32_t mem, void *stream)
{
    const char *fn = "tree_rne_vjp";
    const std::shared_ptr<Tree> t_owner = tree_from_handle(tree);
    Tree *t = t_owner.get();
    RTB_TRACE(fn);
    if (!t) return refuse(fn, "unknown tree handle");
    DeviceScope dscope;
    RTB_TRY(check_batch(fn, q, N, mem, &dscope));
    if (N == 0) return RTBHIP_OK;                            // an empty batch: no pointer is looked at
    if (!gtau) return refuse(fn, "NULL gtau");               // qd / qdd may be NULL (= zeros)
    if (!gq && !gqd && !gqdd) return refuse(fn, "gq, gqd and gqdd are all NULL: there is nothing to compute");
    if (!gravity3) return refuse(fn, "NULL gravity");        // (read on the host, as rtbhip_tree_rne's)
    if (!launch_tree_rne_vjp) return refuse(fn, "not built into this library");
    const DevGroup *groups = nullptr;
    RTB_TRY(tree_device_groups(t, &groups));
    const size_t bytes = (size_t)N * t->n * 8;
    Staged st(mem, stream);
    const double *dq = st.in(q, bytes), *dqd = st.in(qd, bytes), *dqdd = st.in(qdd, bytes), *dg = st.in(gtau, bytes);
    double *dgq = st.out(gq, bytes), *dgqd = st.out(gqd, bytes), *dgqdd = st.out(gqdd, bytes);
    RTB_TRY(st.status());
    return st.finish(launch_tree_rne_vjp(t, groups, dq, dqd, dqdd, N, gravity3, dg, dgq, dgqd, dgqdd, st.stream()));
}

int rtbhip_inertia(rtbhip_dyn_t dyn, const double *q, int64_t N, double *M, int32_t mem, void *stream)
{
    return dyn_entry("inertia", dyn, 0, q, nullptr, nullptr, N, nullptr, M, mem, stream);
}

// the gradient of a loss on rtbhip_inertia's matrices with respect to q (k_inertia_vjp)
int rtbhip_inertia_vjp(rtbhip_dyn_t dyn, const double *q, int64_t N, const double *gM, double *gq, int32_t mem, void *stream)
{
    const char *fn = "inertia_vjp";
    RTB_TRACE(fn);
    const std::shared_ptr<Dyn> d_owner = dyn_from_handle(dyn);
    Dyn *d = d_owner.get();
    if (!d) return refuse(fn, "unknown dyn handle");
    DeviceScope dscope;
    RTB_TRY(check_batch(fn, q, N, mem, &dscope));
    if (N == 0) return RTBHIP_OK;                            // an empty batch: no pointer is looked at
    if (!gM) return refuse(fn, "NULL gM");
    if (!gq) return refuse(fn, "NULL gq");
    if (d->n < 1 || d->n > 16) return refuse(fn, "chains of 1..16 joints", RTBHIP_ELIMIT);          // rtbhip_inertia's built-in sizes
    for (const DevLink &l : d->links)
        if (l.sigma != 0) return refuse(fn, "chain has a prismatic joint");
    if (!launch_inertia_vjp) return refuse(fn, "not built into this library");
    const DevLink *links = nullptr;
    RTB_TRY(dyn_device_links(d, &links));
    const size_t bytes = (size_t)N * (size_t)d->n * 8;
    Staged st(mem, stream);
    const double *dq = st.in(q, bytes), *dg = st.in(gM, bytes * (size_t)d->n);
    double *dgq = st.out(gq, bytes);
    RTB_TRY(st.status());
    return st.finish(launch_inertia_vjp(d, links, dq, N, dg, dgq, st.stream()));
}

int rtbhip_coriolis(rtbhip_dyn_t dyn, const double *q, const double *qd, int64_t N, double *Cm, int32_t mem, void *stream)
{
    return dyn_entry("coriolis", dyn, 1, q, qd, nullptr, N, nullptr, Cm, mem, stream);
}

// the gradient of a loss on rtbhip_coriolis's matrices with respect to q and qd (k_coriolis_vjp); gq or gqd NULL: not wanted
int rtbhip_coriolis_vjp(rtbhip_dyn_t dyn, const double *q, const double *qd, int64_t N, const double *gC, double *gq, double *gqd, int32_t mem,
                        void *stream)
{
    const char *fn = "coriolis_vjp";
    RTB_TRACE(fn);
    const std::shared_ptr<Dyn> d_owner = dyn_from_handle(dyn);
    Dyn *d = d_owner.get();
    if (!d) return refuse(fn, "unknown dyn handle");
    DeviceScope dscope;
    RTB_TRY(check_batch(fn, q, N, mem, &dscope));
    if (N == 0) return RTBHIP_OK;                            // an empty batch: no pointer is looked at
    if (!qd) return refuse(fn, "NULL input with N > 0");
    if (!gC) return refuse(fn, "NULL gC");
    if (!gq && !gqd) return refuse(fn, "NULL gq and NULL gqd");
    if (d->n < 1 || d->n > 16) return refuse(fn, "chains of 1..16 joints", RTBHIP_ELIMIT);          // rtbhip_coriolis's built-in sizes
    for (const DevLink &l : d->links)
        if (l.sigma != 0) return refuse(fn, "chain has a prismatic joint");
    if (!launch_coriolis_vjp) return refuse(fn, "not built into this library");
    const DevLink *links = nullptr;
    RTB_TRY(dyn_device_links(d, &links));
    const size_t bytes = (size_t)N * (size_t)d->n * 8;
    Staged st(mem, stream);
    const double *dq = st.in(q, bytes), *dqd = st.in(qd, bytes), *dg = st.in(gC, bytes * (size_t)d->n);
    double *dgq = gq ? st.out(gq, bytes) : nullptr, *dgqd = gqd ? st.out(gqd, bytes) : nullptr;
    RTB_TRY(st.status());
    return st.finish(launch_coriolis_vjp(d, links, dq, dqd, N, dg, dgq, dgqd, st.stream()));
}

int rtbhip_accel(rtbhip_dyn_t dyn, const double *q, const double *qd, const double *torque, int64_t N,
                 const double *grav3, double *qdd, int32_t mem, void *stream)
{
    return dyn_entry("accel", dyn, 2, q, qd, torque, N, grav3, qdd, mem, stream);
}

int rtbhip_tree_inertia(rtbhip_tree_t tree, const double *q, int64_t N, double *M, int32_t mem, void *stream)
{
    return tree_dyn_entry("tree_inertia", tree, 0, q, nullptr, nullptr, N, nullptr, M, mem, stream);
}

// the gradient of a loss on rtbhip_tree_inertia's matrices with respect to q (k_tree_inertia_vjp)
int rtbhip_tree_inertia_vjp(rtbhip_tree_t tree, const double *q, int64_t N, const double *gM, double *gq, int32_t mem, void *stream)
{
    const char *fn = "tree_inertia_vjp";
    const std::shared_ptr<Tree> t_owner = tree_from_handle(tree);
    Tree *t = t_owner.get();
    RTB_TRACE(fn);
    if (!t) return refuse(fn, "unknown tree handle");
    DeviceScope dscope;
    RTB_TRY(check_batch(fn, q, N, mem, &dscope));
    if (N == 0) return RTBHIP_OK;                            // an empty batch: no pointer is looked at
    if (!gM) return refuse(fn, "NULL gM");
    if (!gq) return refuse(fn, "NULL gq");
    if (t->n < 1 || t->n > 20) return refuse(fn, "robots of 1..20 joints", RTBHIP_ELIMIT);          // rtbhip_tree_inertia's built-in sizes
    for (int j = 0; j < t->n; ++j)
        if (jm_jq(t->groups[j].jmeta) != j)
            return refuse(fn, "the robot is not numbered in group order (joint j of the q row must be moved by link group j)");
    if (!launch_tree_inertia_vjp) return refuse(fn, "not built into this library");
    const DevGroup *groups = nullptr;
    RTB_TRY(tree_device_groups(t, &groups));
    const size_t bytes = (size_t)N * (size_t)t->n * 8;
    Staged st(mem, stream);
    const double *dq = st.in(q, bytes), *dg = st.in(gM, bytes * (size_t)t->n);
    double *dgq = st.out(gq, bytes);
    RTB_TRY(st.status());
    return st.finish(launch_tree_inertia_vjp(t, groups, dq, N, dg, dgq, st.stream()));
}

/* operational-space dynamics from a supplied Jacobian (k_opspace / k_tree_opspace): device pointers only, like rtbhip_ik_vjp */
int rtbhip_opspace(rtbhip_dyn_t dyn, const double *q, const double *J, int64_t N, const double *grav3, int32_t axes_mask, double *Mx, double *Gx,
                   double *asada, void *stream)
{
    const char *fn = "opspace";
    const std::shared_ptr<Dyn> d_owner = dyn_from_handle(dyn);
    Dyn *d = d_owner.get();
    RTB_TRACE(fn);
    if (!d) return refuse(fn, "unknown dyn handle");
    bool go = false;
    RTB_TRY(opspace_check(fn, d->n, q, J, N, grav3, axes_mask, Mx, Gx, asada, &go));
    if (!go) return RTBHIP_OK;
    if (!launch_opspace) return refuse(fn, "not built into this library");
    DeviceScope dscope;
    RTB_TRY(dscope.enter_for(fn, q));
    const DevLink *links = nullptr;
    RTB_TRY(dyn_device_links(d, &links));
    return launch_opspace(d, links, q, J, N, grav3, axes_mask, Mx, Gx, asada, (hipStream_t)stream);
}

int rtbhip_tree_opspace(rtbhip_tree_t tree, const double *q, const double *J, int64_t N, const double *grav3, int32_t axes_mask, double *Mx, double *Gx,
                        double *asada, void *stream)
{
    const char *fn = "tree_opspace";
    const std::shared_ptr<Tree> t_owner = tree_from_handle(tree);
    Tree *t = t_owner.get();
    RTB_TRACE(fn);
    if (!t) return refuse(fn, "unknown tree handle");
    bool go = false;
    RTB_TRY(opspace_check(fn, t->n, q, J, N, grav3, axes_mask, Mx, Gx, asada, &go));
    for (int j = 0; j < t->n; ++j)
        if (jm_jq(t->groups[j].jmeta) != j)
            return refuse(fn, "the robot is not numbered in group order (joint j of the q row must be moved by link group j)");
    if (!go) return RTBHIP_OK;
    if (!launch_tree_opspace) return refuse(fn, "not built into this library");
    DeviceScope dscope;
    RTB_TRY(dscope.enter_for(fn, q));
    const DevGroup *groups = nullptr;
    RTB_TRY(tree_device_groups(t, &groups));
    return launch_tree_opspace(t, groups, q, J, N, grav3, axes_mask, Mx, Gx, asada, (hipStream_t)stream);
}

int rtbhip_tree_coriolis(rtbhip_tree_t tree, const double *q, const double *qd, int64_t N, double *Cm, int32_t mem, void *stream)
{
    return tree_dyn_entry("tree_coriolis", tree, 1, q, qd, nullptr, N, nullptr, Cm, mem, stream);
}

// the gradient of a loss on rtbhip_tree_coriolis's matrices with respect to q and qd (k_tree_coriolis_vjp); gq or gqd NULL: not wanted
int rtbhip_tree_coriolis_vjp(rtbhip_tree_t tree, const double *q, const double *qd, int64_t N, const double *gC, double *gq, double *gqd, int32_t mem,
                             void *stream)
{
    const char *fn = "tree_coriolis_vjp";
    const std::shared_ptr<Tree> t_owner = tree_from_handle(tree);
    Tree *t = t_owner.get();
    RTB_TRACE(fn);
    if (!t) return refuse(fn, "unknown tree handle");
    DeviceScope dscope;
    RTB_TRY(check_batch(fn, q, N, mem, &dscope));
    if (N == 0) return RTBHIP_OK;                            // an empty batch: no pointer is looked at
    if (!qd) return refuse(fn, "NULL input with N > 0");
    if (!gC) return refuse(fn, "NULL gC");
    if (!gq && !gqd) return refuse(fn, "NULL gq and NULL gqd");
    if (t->n < 1 || t->n > 20) return refuse(fn, "robots of 1..20 joints", RTBHIP_ELIMIT);          // rtbhip_tree_coriolis's built-in sizes
    for (int j = 0; j < t->n; ++j)
        if (jm_jq(t->groups[j].jmeta) != j)
            return refuse(fn, "the robot is not numbered in group order (joint j of the q row must be moved by link group j)");
    if (!launch_tree_coriolis_vjp) return refuse(fn, "not built into this library");
    const DevGroup *groups = nullptr;
    RTB_TRY(tree_device_groups(t, &groups));
    const size_t bytes = (size_t)N * (size_t)t->n * 8;
    Staged st(mem, stream);
    const double *dq = st.in(q, bytes), *dqd = st.in(qd, bytes), *dg = st.in(gC, bytes * (size_t)t->n);
    double *dgq = gq ? st.out(gq, bytes) : nullptr, *dgqd = gqd ? st.out(gqd, bytes) : nullptr;
    RTB_TRY(st.status());
    return st.finish(launch_tree_coriolis_vjp(t, groups, dq, dqd, N, dg, dgq, dgqd, st.stream()));
}

int rtbhip_tree_accel(rtbhip_tree_t tree, const double *q, const double *qd, const double *torque, int64_t N,
                      const double *gravity3, double *qdd, int32_t mem, void *stream)
{
    return tree_dyn_entry("tree_accel", tree, 2, q, qd, torque, N, gravity3, qdd, mem, stream);
}

int rtbhip_fleet_fkine_jacob(const rtbhip_chain_t *chains, int32_t n_chains, const double *const *q,
                             const int64_t *N, int32_t frame, double *const *T, double *const *J,
                             int32_t mem, void *stream)
{
    return fleet_entry(chains, n_chains, q, N, frame, T, J, mem, stream, false);
}

int rtbhip_fleet_fkine_jacob_packed(const rtbhip_chain_t *chains, int32_t n_chains, const double *const *q,
                                    const int64_t *N, int32_t frame, double *const *TJ, int32_t mem, void *stream)
{
    return fleet_entry(chains, n_chains, q, N, frame, TJ, nullptr, mem, stream, true);
}

int rtbhip_host_alloc(uint64_t bytes, void **ptr)
{
    if (!ptr) { set_error("host_alloc: NULL out"); return RTBHIP_EINVAL; }
    return host_alloc((size_t)bytes, ptr);
}

int rtbhip_host_free(void *ptr) { return host_free(ptr); }

int rtbhip_shard_range(int64_t N, int32_t rank, int32_t world, int64_t *begin, int64_t *count)
{
    if (N < 0 || world < 1 || rank < 0 || rank >= world || !begin || !count) { set_error("shard_range: bad argument"); return RTBHIP_EINVAL; }
    int64_t base = N / world, extra = N % world;
    *count = base + (rank < extra ? 1 : 0);
    *begin = base * rank + (rank < extra ? rank : extra);
    return RTBHIP_OK;
}

int rtbhip_last_launch(int32_t *grid, int32_t *block, int32_t *lds_bytes)
{
    if (grid) *grid = g_last_launch[0];
    if (block) *block = g_last_launch[1];
    if (lds_bytes) *lds_bytes = g_last_launch[2];
    return RTBHIP_OK;
}

int rtbhip_stream_probe(const double *src, int64_t read_doubles, double *dst, int64_t write_doubles, void *stream)
{
    if ((read_doubles > 0 && !src) || (write_doubles > 0 && !dst) || read_doubles < 0 || write_doubles < 0) { set_error("stream_probe: bad argument"); return RTBHIP_EINVAL; }
    DeviceScope dscope;
    RTB_TRY(check_batch("stream_probe", dst ? dst : src, 1, RTBHIP_MEM_DEVICE, &dscope));
    return launch_stream_probe(src, read_doubles, dst, write_doubles, (hipStream_t)stream);
}

int rtbhip_tune(const char *key, int32_t value)
{
    if (!key) { set_error("tune: NULL key"); return RTBHIP_EINVAL; }
    kin_tune(key, value);
    rne_tune(key, value);
    ik_tune(key, value);
    partial_tune(key, value);
    if (std::string(key) == "rne_pszero") g_rne_pszero = value != 0;
    hostpipe_tune(key, value);
    shard_tune(key, value);
    tree_tune(key, value);
    jit_tune(key, value);
    return RTBHIP_OK;
}

// ---- run-time instantiation (jit.cpp)
int rtbhip_jit_stats(rtbhip_jit_info *out)
{
    if (!out) { set_error("jit_stats: NULL out"); return RTBHIP_EINVAL; }
    jit_stats(out);
    return RTBHIP_OK;
}
int rtbhip_jit_wait(double timeout_s) { return jit_wait(timeout_s); }
int rtbhip_jit_compile(const char *unit, const char *expr, const char *arch, int64_t *code_bytes, double *seconds, int32_t *from_disk)
{
    if (!unit || !expr || !arch) { set_error("jit_compile: NULL argument"); return RTBHIP_EINVAL; }
    size_t cb = 0;
    double sec = 0.0;
    int fd = 0;
    // "unit" may carry generated source after a newline (a tree's knowledge type): "tree_kernels.hip\nnamespace rtbhip { struct ... }"
    const std::string u = unit;
    const size_t nl = u.find('\n');
    const std::string file = nl == std::string::npos ? u : u.substr(0, nl), pre = nl == std::string::npos ? std::string() : u.substr(nl + 1);
    const int rc = jit_compile_now(file.c_str(), expr, arch, &cb, &sec, &fd, pre.c_str());
    if (code_bytes) *code_bytes = (int64_t)cb;
    if (seconds) *seconds = sec;
    if (from_disk) *from_disk = fd;
    return rc;
}
int rtbhip_jit_prepare(int32_t kind, uint64_t handle)
{
    if (kind == 0) { auto c = chain_from_handle(handle); if (!c) return RTBHIP_EINVAL; jit_request_chain(c.get(), true); }
    else if (kind == 1) { auto d = dyn_from_handle(handle); if (!d) return RTBHIP_EINVAL; jit_request_dyn(d.get(), true, true); }
    else if (kind == 2) { auto t = tree_from_handle(handle); if (!t) return RTBHIP_EINVAL; jit_request_tree(t.get(), true, true); }
    else { set_error("jit_prepare: kind must be 0 (chain), 1 (dyn) or 2 (tree)"); return RTBHIP_EINVAL; }
    return RTBHIP_OK;
}
int rtbhip_jit_names(int32_t kind, uint64_t handle, char *buf, int64_t cap)
{
    if (!buf || cap < 1) { set_error("jit_names: bad buffer"); return RTBHIP_EINVAL; }
    std::vector<std::string> names;
    std::string pre;
    if (kind == 0) { auto c = chain_from_handle(handle); if (!c) return RTBHIP_EINVAL; names = ik_jit_names(c.get()); }
    else if (kind == 1) { auto d = dyn_from_handle(handle); if (!d) return RTBHIP_EINVAL; names = rne_jit_names(d.get()); }
    else if (kind == 2) {
        auto t = tree_from_handle(handle);
        if (!t) return RTBHIP_EINVAL;
        names = tree_jit_names(t.get());
        if (!names.empty()) { std::string tn; pre = tree_jit_knowledge(t.get(), &tn); }
    } else { set_error("jit_names: kind must be 0 (chain), 1 (dyn) or 2 (tree)"); return RTBHIP_EINVAL; }
    std::string all;
    for (const std::string &n : names) all += n + "\n";
    if (!pre.empty()) all += "\f" + pre;            // after a form feed: the generated knowledge type the tree's expressions refer to
    std::snprintf(buf, (size_t)cap, "%s", all.c_str());
    return RTBHIP_OK;
}

}  // extern "C"
