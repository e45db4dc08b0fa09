// fmha_api.cpp — the C ABI of libpaged-attention.so (declared in include/paged_attn.h).
//
// Re-implements the reference's L3 boundary (csrc/paged_attn.cpp:6-568): parameter packing
// (set_params_fprop_strided :6-126), the split heuristic (:128-163), split scratch (:165-196)
// and the three entry points (:310-568) — plus fmha_bwd / varlen / _ex entries the reference
// lacks.  Differences by design:
//   * no exceptions or exit() cross the ABI: failures set a thread-local error and return;
//   * split scratch comes from a cached per-(device, stream) pool — no hipMalloc/hipFree per call
//     (the reference mallocs every call and leaks, paged_attn.cpp:186-189,557-561);
//   * the current device is used (the reference queries device 0, :527-528);
//   * LSE is written whenever a pointer is given.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "../../include/paged_attn.h"
#include "fmha_launch.h"

using namespace xfa;

namespace xfa {
Options& options() {
    static Options o;
    return o;
}
thread_local char g_last_kernel[160] = "";   // kernel + schedule of this thread's last forward
void note_launch(const char* kernel, int persistent, int xcdq, unsigned gx, unsigned gy, unsigned gz, int block) {
    snprintf(g_last_kernel, sizeof(g_last_kernel), "%s persistent=%d xcdq=%d grid=%ux%ux%u block=%d",
             kernel, persistent, xcdq, gx, gy, gz, block);
}
void note_body(const char* body) {
    const size_t n = strlen(g_last_kernel);
    snprintf(g_last_kernel + n, sizeof(g_last_kernel) - n, " body=%s", body);
}
thread_local SinkMech g_sink_mech = kSinkNone;   // how this thread's last forward applied its sink
void note_sink(SinkMech mech) { g_sink_mech = mech; }
}  // namespace xfa

namespace {

thread_local std::string g_err;
thread_local int g_status = 0;
thread_local int g_last_splits = 0;     // split count of this thread's last forward launch

void clear_error() { g_err.clear(); g_status = 0; }
// forward entries: also forget the last forward's kernel / splits, so a call that fails
// validation or launches nothing reports "" / 0 (fmha_last_kernel's contract)
void begin_fwd() { clear_error(); g_last_kernel[0] = 0; g_last_splits = 0; g_sink_mech = kSinkNone; }
bool fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
bool fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
    g_status = code;
    return false;
}
#define REQUIRE(cond, ...) do { if (!(cond)) { fail(1, __VA_ARGS__); return; } } while (0)

bool hip_ok(hipError_t e, const char* what) {
    if (e == hipSuccess) return true;
    return fail(2, "%s: %s", what, hipGetErrorString(e));
}

// ---------------------------------------------------------------- scratch pool ---------
// One growable device buffer per (device, stream).  Work on a stream is ordered, so reuse
// by the next call on the same stream is safe; growth frees the old block (hipFree waits).
struct PoolEntry { void* ptr = nullptr; size_t bytes = 0; };
std::mutex g_pool_mu;
std::map<std::pair<int, hipStream_t>, PoolEntry> g_pool;

void* pool_get(hipStream_t st, size_t bytes) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return nullptr;
    std::lock_guard<std::mutex> lk(g_pool_mu);
    PoolEntry& e = g_pool[{dev, st}];
    if (e.bytes >= bytes) return e.ptr;
    if (e.ptr) { hipStreamSynchronize(st); hipFree(e.ptr); e.ptr = nullptr; e.bytes = 0; }
    size_t want = bytes + (bytes >> 3) + 4096;
    if (hipMalloc(&e.ptr, want) != hipSuccess) { e.ptr = nullptr; return nullptr; }
    e.bytes = want;
    return e.ptr;
}

// Item counters of the dynamic persistent forward (one pair of ints per (device, stream),
// zeroed once; the kernel's last workgroup resets them, so stream order keeps them valid).
std::map<std::pair<int, hipStream_t>, int*> g_ctr;
int* counter_get(hipStream_t st) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return nullptr;
    std::lock_guard<std::mutex> lk(g_pool_mu);
    int*& c = g_ctr[{dev, st}];
    if (!c) {
        if (hipMalloc(&c, 256) != hipSuccess) { c = nullptr; return nullptr; }
        if (hipMemsetAsync(c, 0, 256, st) != hipSuccess) { (void)hipFree(c); c = nullptr; return nullptr; }
    }
    return c;
}

// Split-arrival counters of the folded decode combine: >= n ints per (device, stream), zeroed
// when (re)allocated; every launch leaves them zero (the merging wave resets its counter).
std::map<std::pair<int, hipStream_t>, std::pair<int*, int>> g_dec_ctr;
int* dec_counters(hipStream_t st, int n) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return nullptr;
    std::lock_guard<std::mutex> lk(g_pool_mu);
    auto& e = g_dec_ctr[{dev, st}];
    if (e.second >= n) return e.first;
    if (e.first) { hipStreamSynchronize(st); (void)hipFree(e.first); e.first = nullptr; e.second = 0; }
    const int want = std::max(n, 1024);
    if (hipMalloc(&e.first, (size_t)want * 4) != hipSuccess) { e.first = nullptr; return nullptr; }
    if (hipMemsetAsync(e.first, 0, (size_t)want * 4, st) != hipSuccess) { (void)hipFree(e.first); e.first = nullptr; return nullptr; }
    e.second = want;
    return e.first;
}

// CU count per device (a process may drive several GPUs; cached per device id)
int num_cus(int dev) {
    static std::mutex mu;
    static std::map<int, int> cache;
    std::lock_guard<std::mutex> lk(mu);
    auto it = cache.find(dev);
    if (it != cache.end()) return it->second;
    int n = 0;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
    cache[dev] = n;
    return n;
}
int current_device() {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) dev = 0;
    return dev;
}

// Kernels address one sequence's rows of one tensor with 32-bit byte offsets from a buffer
// descriptor (and mark skipped lanes with kOOB = 0x7FFFFF00), so one sequence's slab of any
// tensor must stay below that (the reference's 64-bit index_t has no such limit; a slab this
// large is >= 256k tokens x 32 heads x d128 in bf16).
constexpr int64_t kMaxSlabBytes = 0x7FFFFF00LL;
bool slab_ok(const char* what, int64_t rows, int64_t row_elems, int esz) {
    const int64_t bytes = rows * row_elems * esz;
    if (bytes < kMaxSlabBytes) return true;
    return fail(1, "%s: one sequence spans %lld bytes (%lld rows x %lld elements); this build "
                "addresses a sequence with 32-bit offsets and supports < %lld bytes",
                what, (long long)bytes, (long long)rows, (long long)row_elems, (long long)kMaxSlabBytes);
}

// Reference heuristic (paged_attn.cpp:128-163): the smallest split count whose wave
// efficiency reaches 85% of the best, capped at 128.  "SMs" = CUs x resident workgroups.
int num_splits_heuristic(int work_blocks, int slots, int n_blocks, int max_splits) {
    if (work_blocks >= 0.8f * slots) return 1;
    max_splits = std::min(std::min(max_splits, slots), n_blocks);
    if (max_splits <= 1) return 1;
    auto cdiv = [](int a, int b) { return (a + b - 1) / b; };
    std::vector<float> eff(max_splits + 1, 0.f);
    float best = 0.f;
    for (int s = 1; s <= max_splits; ++s) {
        if (s > 1 && cdiv(n_blocks, s) == cdiv(n_blocks, s - 1)) continue;
        float waves = float(work_blocks * s) / slots;
        eff[s] = waves / std::ceil(waves);
        best = std::max(best, eff[s]);
    }
    for (int s = 1; s <= max_splits; ++s) {
        if (s > 1 && cdiv(n_blocks, s) == cdiv(n_blocks, s - 1)) continue;
        if (eff[s] >= 0.85f * best) return s;
    }
    return 1;
}

int hd_bucket(int d) { return d <= 64 ? 64 : (d <= 128 ? 128 : 256); }

hipError_t dispatch_fwd(const FwdParams& p, bool bf16, hipStream_t st) {
    const int hd = hd_bucket(p.d);
    if (hd == 64) return bf16 ? launch_fwd_hd64_bf16(p, st) : launch_fwd_hd64_f16(p, st);
    if (hd == 128) return bf16 ? launch_fwd_hd128_bf16(p, st) : launch_fwd_hd128_f16(p, st);
    if (hd == 256) return bf16 ? launch_fwd_hd256_bf16(p, st) : launch_fwd_hd256_f16(p, st);
    return hipErrorInvalidValue;
}

hipError_t dispatch_bwd(const BwdParams& p, bool bf16, hipStream_t st) {
    const int hd = hd_bucket(p.d);
    if (hd == 64) return bf16 ? launch_bwd_hd64_bf16(p, st) : launch_bwd_hd64_f16(p, st);
    if (hd == 128) return bf16 ? launch_bwd_hd128_bf16(p, st) : launch_bwd_hd128_f16(p, st);
    if (hd == 256) return bf16 ? launch_bwd_hd256_bf16(p, st) : launch_bwd_hd256_f16(p, st);
    return hipErrorInvalidValue;
}

// Score scaling as set_params_fprop_strided (paged_attn.cpp:93-102): with softcap the
// kernel computes tanh(s * scale / cap) and then scales by cap.
template <typename P>
void set_scales(P& p, float softmax_scale, float softcap) {
    float scale_softmax;
    if (softcap > 0.f) { p.softcap_pre = softmax_scale / softcap; scale_softmax = softcap; }
    else { p.softcap_pre = 0.f; scale_softmax = softmax_scale; }
    p.scale_log2 = scale_softmax * 1.4426950408889634f;
    p.alibi_mul = 1.f / scale_softmax;
}

template <typename P>
static LseAlibiParams lse_alibi_params(const P& p, float sign) {
    LseAlibiParams a{};
    a.src = p.lse; a.dst = nullptr; a.sign = sign;
    a.alibi = p.alibi; a.alibi_bstride = p.alibi_bstride;
    a.b = p.b; a.h = p.h; a.seqlen_q = p.seqlen_q; a.seqlen_k = p.seqlen_k;
    a.cu_seqlens_q = p.cu_seqlens_q; a.cu_seqlens_k = p.cu_seqlens_k;
    a.lse_batch = p.lse_batch; a.lse_head = p.lse_head;
    return a;
}
static LseAlibiParams lse_alibi_params(const FwdParams& p, float sign) {
    LseAlibiParams a = lse_alibi_params<FwdParams>(p, sign);
    a.dst = p.lse;
    a.seqused_k = p.seqused_k; a.leftpad_k = p.leftpad_k;
    return a;
}

// Window normalisation (paged_attn.cpp:116-120): causal <=> wl < 0 && wr == 0.
// Returns the reference's is_causal (before the normalisation), which picks its ALiBi form.
bool set_windows(int& wl, int& wr, int seqlen_k) {
    const bool causal = wl < 0 && wr == 0;
    if (wl < 0 && wr >= 0) wl = seqlen_k;
    if (wl >= 0 && wr < 0) wr = seqlen_k;
    return causal;
}

bool check_common(const void* q, const void* k, const void* v, const void* o, int b, int h,
                  int hk, int d) {
    if (!q || !k || !v || !o) return fail(1, "q/k/v/o must be non-null device pointers");
    if (b <= 0) return fail(1, "batch size must be positive (got %d)", b);
    if (h <= 0 || hk <= 0 || h % hk != 0)
        return fail(1, "Number of heads in key/value must divide number of heads in query (h=%d, hk=%d)", h, hk);
    if (d <= 0 || d % 8 != 0) return fail(1, "head_size must be a positive multiple of 8 (got %d)", d);
    if (d > 256) return fail(1, "FlashAttention forward only supports head dimension at most 256 (got %d)", d);
    // the kernels move 16-byte chunks (b128 buffer loads, LDS-DMA, 16-byte stores)
    if (((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)o) & 15)
        return fail(1, "q/k/v/o must be 16-byte aligned device pointers");
    return true;
}

// ---- the forward packer: what every entry fills the same way, then one layout each ----------
// pointers, shape, windows, scales, ALiBi
void fwd_common(FwdParams& p, void* q, void* k, void* v, void* o, void* lse, int b, int h, int hk,
                int d, int seqlen_q, int seqlen_k, int wl, int wr, float softmax_scale,
                float softcap, const void* alibi, int alibi_bstride, const float* sink = nullptr) {
    p.sink = sink;
    p.q = q; p.k = k; p.v = v; p.o = o; p.lse = (float*)lse;
    p.b = b; p.h = h; p.hk = hk; p.group = h / hk; p.d = d;
    p.seqlen_q = seqlen_q; p.seqlen_k = seqlen_k;
    p.alibi_causal = set_windows(wl, wr, seqlen_k);
    p.wl = wl; p.wr = wr;
    set_scales(p, softmax_scale, softcap);
    p.alibi = (const float*)alibi; p.alibi_bstride = alibi_bstride;
}

// contiguous rows [.., heads, d] (element strides; fp8 elements are bytes, so q/k/v strides are
// byte strides too), LSE [.., seqlen_q]; the batch strides are the layout's
void row_strides(FwdParams& p, int h, int hk, int d) {
    p.q_row = (int64_t)h * d;  p.q_head = d;
    p.k_row = (int64_t)hk * d; p.k_head = d;
    p.v_row = (int64_t)hk * d; p.v_head = d;
    p.o_row = (int64_t)h * d;  p.o_head = d;
}
void dense_strides(FwdParams& p, int sq, int sk, int h, int hk, int d) {
    row_strides(p, h, hk, d);
    p.q_batch = p.o_batch = (int64_t)sq * h * d;
    p.k_batch = p.v_batch = (int64_t)sk * hk * d;
    p.lse_batch = (int64_t)h * sq; p.lse_head = sq;
}
// packed rows: no batch stride (cu_seqlens give the offsets); unpadded LSE [num_heads, total_q]
// (export.cpp:827): index = h * total_q + q_off + pos
void packed_strides(FwdParams& p, int h, int hk, int d, int total_q) {
    row_strides(p, h, hk, d);
    p.q_batch = p.o_batch = p.k_batch = p.v_batch = 0;
    p.lse_batch = 0; p.lse_head = total_q;
}
// paged K/V: the "batch" stride is the page stride (paged_attn.cpp:506-507); pages are per
// sequence, so there is no k offset
void paged_kv(FwdParams& p, const void* block_table, int bt_stride, int page, int hk, int d) {
    p.block_table = (const int*)block_table;
    p.bt_stride = bt_stride;
    p.page_size = page;
    p.k_batch = p.v_batch = (int64_t)page * hk * d;
}

// Dropout RNG state of the calling thread (fmha_set_rng_state); read by every forward /
// backward call with p_dropout > 0.
thread_local uint64_t g_seed = 0, g_offset = 0;
// fmha_set_rng_state_device: the key read on the device (graph capture), and where a forward
// writes the key it used
thread_local const int64_t* g_seed_ptr = nullptr;
thread_local const int64_t* g_offset_ptr = nullptr;
thread_local uint64_t g_offset_add = 0;
thread_local int64_t* g_rng_out = nullptr;
// The device key is consumed by the next compute entry whatever its outcome (a call that fails
// validation before set_dropout must not leave a stale rng_out for a later one)
struct DevRngScope {
    ~DevRngScope() {
        g_seed_ptr = g_offset_ptr = nullptr;
        g_rng_out = nullptr;
    }
};

template <typename P>
bool set_dropout(P& p, float p_dropout, float softcap) {
    if (!(p_dropout >= 0.f && p_dropout < 1.f)) return fail(1, "p_dropout must be in [0, 1) (got %g)", p_dropout);
    // the reference's rule (export.cpp:515,737; flash_api_hip.cpp:400,606,895,1128)
    if (softcap > 0.f && p_dropout > 0.f) return fail(1, "Softcapping does not support dropout for now");
    p.drop = p_dropout > 0.f;
    if (!p.drop) return true;
    const float keep = 1.f - p_dropout;                   // paged_attn.cpp:106-113
    p.keep_thr = (uint32_t)std::floor(keep * 255.0);
    p.rp_keep = 1.f / keep;
    p.seed = g_seed;
    p.offset = g_seed_ptr ? g_offset_add : g_offset;
    p.seed_ptr = g_seed_ptr;
    p.offset_ptr = g_offset_ptr;
    p.rng_out = g_rng_out;
    return true;
}

// return_softmax: the dropped-out softmax [b, h, round128(sq), round128(sk)] after the forward
void run_sdmask(const FwdParams& p, void* s, bool bf16, hipStream_t st) {
    const int sq_r = (p.seqlen_q + 127) / 128 * 128, sk_r = (p.seqlen_k + 127) / 128 * 128;
    hip_ok(bf16 ? launch_sdmask_bf16(p, s, sq_r, sk_r, st) : launch_sdmask_f16(p, s, sq_r, sk_r, st),
           "return_softmax launch");
}

// The one place that reads the schedule knobs every forward launch shares.  p.fwd4 carries
// either kernel-choice knob: fwd_w4 on the bf16 / fp16 forward, fp8_w4 on the fp8 one (their
// launchers are separate, so the field never means both).  slack_max: the kernels keep
// P = exp2(S c - m_sc) within 2^fwd_slack, and P is rounded to the type of the PV operand, so the
// slack a launch runs with stops where that type does: 8 for e4m3 (256 < 448), 15 for fp16
// (2^16 rounds to inf), the knob's own 16 for bf16.
void load_schedule(FwdParams& p, const std::atomic<int>& w4, int slack_max) {
    Options& o = options();
    p.device = current_device();
    p.num_cus = num_cus(p.device);
    p.fwd4 = w4.load();
    p.persist_per_cu = o.fwd_persistent.load();
    p.order = o.fwd_order.load();
    p.xcdq = o.fwd_xcdq.load();
    p.max_slack = (float)std::min(o.fwd_slack.load(), slack_max);
}
// ... and takes the item-queue counter where fwd_dyn reaches `dyn_min`; `code`: the status of
// a failed allocation
bool take_item_queue(FwdParams& p, hipStream_t st, int dyn_min, int code) {
    if (options().fwd_dyn.load() < dyn_min) return true;
    p.work_ctr = counter_get(st);
    return p.work_ctr || fail(code, "could not allocate the item-queue counters");
}

void run_fwd(FwdParams& p, bool bf16, hipStream_t st, int num_splits_req) {
    Options& o = options();
    load_schedule(p, o.fwd_w4, bf16 ? 16 : 15);
    p.waves = o.fwd_waves.load();
    p.prio_hi = o.fwd_prio.load();
    p.pipe = o.fwd_pipe.load();
    const int n_blocks = (p.seqlen_k + kBlockN - 1) / kBlockN;
    if (p.drop) num_splits_req = 1;       // no split-KV with dropout (paged_attn.cpp:180)
    int splits = num_splits_req;
    // Decode: the whole GQA group of query rows fits one 32-row MFMA tile -> the split-KV
    // decode kernel (every wave a split, fmha_decode_kernel.h); splits a multiple of 4.
    p.decode = o.fwd_decode.load() && !p.drop && !p.cu_seqlens_q && !p.cu_seqlens_k &&
               p.seqlen_q * p.group <= 32 && hd_bucket(p.d) == p.d && p.d <= 128 &&
               (!p.block_table || p.page_size % 16 == 0);
    if (p.decode) {
        const int tiles = (p.seqlen_k + 31) / 32;
        const int work = p.b * p.hk;
        int zs = num_splits_req > 0 ? (num_splits_req + 3) / 4
                                    : (o.dec_wg_per_cu.load() * p.num_cus + work - 1) / work;
        zs = std::max(1, std::min(zs, std::max(1, tiles / 8)));
        zs = std::min(zs, 32);
        splits = 4 * zs;
        // head-major workgroups (4 or 8 kv heads of one split) when the kv heads divide evenly
        const int hm = o.dec_hmaj.load();
        p.dec_mr = (o.dec_mr.load() == 16 && p.seqlen_q * p.group <= 16) ? 16 : 32;
        p.dec_hmaj = (hm == 2 && p.hk % 8 == 0) ? 2 : (hm >= 1 && p.hk % 4 == 0) ? 1 : 0;
    } else if (p.cu_seqlens_q) {
        splits = 1;  // varlen: single pass (the reference forces it too)
    } else if (splits <= 0) {
        const int work = p.b * p.hk * fwd_num_m_blocks(p.seqlen_q, p.group, p.d, p.waves);
        splits = num_splits_heuristic(work, p.num_cus * 2, n_blocks, 128);
    }
    if (!p.decode) splits = std::max(1, std::min(splits, std::min(128, std::max(1, n_blocks))));
    p.num_splits = splits;
    g_last_splits = splits;
    // Ragged caches (per-sequence lengths): the b * splits slots of a kv-head group are shared
    // in proportion to the sequences' key tiles, up to 128 splits for one sequence
    // (fmha_decode_kernel.h dec_slot); equal lengths give the same splits as without.
    p.dec_bal = p.decode && o.dec_bal.load() && !o.dec_fold.load() && p.dec_hmaj >= 1 &&
                p.seqused_k && p.b >= 2 && p.b <= 64;
    p.dec_slots = p.dec_bal ? p.b * splits : 0;
    p.dec_cap = p.dec_bal ? std::min(p.dec_slots, 128) : 0;
    p.dec_ns = nullptr;
    p.comb_row = o.comb_row.load();
    const int ext = p.dec_bal ? p.dec_cap : splits;   // split extent of the scratch
    // The sink post-pass (a launch that ends in a generated D = 128 body, or in the folded decode
    // merge) reads the LSE the launch wrote: a caller that asked for none gets it in pool scratch,
    // behind the split scratch in the same block (the pool is one block per stream, so two
    // requests would alias).  Rows as the LSE's own layout: packed launches [h, total_q].
    const size_t lse_rows = p.cu_seqlens_q ? (size_t)p.h * p.lse_head : (size_t)p.b * p.h * p.seqlen_q;
    const size_t sink_lse = (p.sink && !p.lse && (p.d == 128 || (p.decode && o.dec_fold.load())))
                                ? lse_rows * sizeof(float) : 0;
    if (splits > 1 || sink_lse) {
        const int hd = hd_bucket(p.d);
        const size_t rows = (size_t)p.b * p.h * p.seqlen_q;
        const size_t obytes = splits > 1 ? (size_t)ext * rows * hd * sizeof(float) : 0;
        const size_t lbytes = splits > 1 ? (size_t)ext * rows * sizeof(float) : 0;
        const size_t nbytes = ((p.dec_bal ? (size_t)p.b * sizeof(int) : 0) + 15) / 16 * 16;
        const size_t bytes = obytes + lbytes + nbytes + sink_lse;
        char* base = (char*)pool_get(st, bytes);
        if (!base) { fail(3, "could not allocate %zu bytes of split scratch", bytes); return; }
        if (splits > 1) {
            p.oaccum = (float*)base;
            p.lseaccum = (float*)(base + obytes);
            if (p.dec_bal) p.dec_ns = (int*)(base + obytes + lbytes);
        }
        if (sink_lse) p.lse = (float*)(base + obytes + lbytes + nbytes);
    }
    p.dec_ctr = nullptr;
    if (p.decode && o.dec_fold.load()) {
        p.dec_ctr = dec_counters(st, p.b * p.hk);
        if (!p.dec_ctr) { fail(3, "could not allocate the decode split counters"); return; }
    }
    // dynamic item queue: ragged (varlen) row blocks balance across CUs as they finish; also the
    // dense D = 128 launches without a right window (the 16x16x32 ping-pong body), whose equal
    // items ran 0.7-1.0 % faster from the per-XCD queues than from the static XCD pairs on two
    // leases (causal launches keep the pairs, which balance their item sizes),
    // and the D = 128 launches with a left window, whose row blocks past the window's width all
    // carry the same work, so the pairs unbalance them (+7 % at (1023, 0), +4 % at (255, 0);
    // profiles/r06_window_dyn_ab.log), and the non-causal ALiBi launches (32x32x16 body, +0.5 to
    // +3.2 % on two boxes; non-causal softcap measured -0.4 % and keeps the pairs:
    // r06_noncausal_feat_ab.log)
    const bool nc16 = p.d == 128 && p.wr < 0 && p.fwd4 == 4 && !p.alibi && !(p.softcap_pre > 0.f);
    const bool ncab = p.d == 128 && p.wr < 0 && p.fwd4 == 4 && p.alibi;
    const bool win = p.d == 128 && p.fwd4 == 4 && p.wl >= 0 && p.wl < p.seqlen_k;  // causal: wl = seqlen_k
    const int dyn_min = (p.cu_seqlens_q || nc16 || ncab || win) ? 1 : 2;
    if (!p.decode && splits == 1 && !take_item_queue(p, st, dyn_min, 3)) return;
    if (!hip_ok(dispatch_fwd(p, bf16, st), "forward launch")) return;
    // causal ALiBi: the LSE in the reference's convention (+slope key, mask_hip.h:163-164)
    if (p.lse && p.alibi && p.alibi_causal) hip_ok(launch_lse_alibi(lse_alibi_params(p, +1.f), st), "LSE ALiBi pass");
    if (!p.sink) return;
    // the launcher recorded which mechanism applies the sink (fmha_launch.h SinkMech)
    if (g_sink_mech == kSinkPass) {
        SinkPassParams sp{};
        sp.o = p.o; sp.lse = p.lse; sp.sink = p.sink;
        sp.o_batch = p.o_batch; sp.o_row = p.o_row; sp.o_head = p.o_head;
        sp.lse_batch = p.lse_batch; sp.lse_head = p.lse_head;
        sp.b = p.cu_seqlens_q ? 1 : p.b;
        sp.rows = p.cu_seqlens_q ? (int)p.lse_head : p.seqlen_q;    // packed: total_q rows
        sp.h = p.h; sp.d = p.d;
        if (!hip_ok(launch_sink_pass(sp, !bf16, st), "sink post-pass")) return;
    }
    static const char* const kMech[] = {"", " sink=epilogue", " sink=combine", " sink=pass"};
    strncat(g_last_kernel, kMech[g_sink_mech], sizeof(g_last_kernel) - strlen(g_last_kernel) - 1);
}

// An attention sink (the _sink entries; null: none): not with ALiBi (the kernels' causal-ALiBi
// frame shifts a row's scores by a constant, and a sink is not shift-invariant), dropout or
// return_softmax
bool check_sink(const float* sink, const void* alibi, float p_dropout, const void* s_dmask) {
    if (!sink) return true;
    if (((uintptr_t)sink) & 3) return fail(1, "sink must be a 4-byte aligned device pointer (fp32 [num_heads])");
    if (alibi) return fail(1, "an attention sink does not support ALiBi");
    if (p_dropout > 0.f || s_dmask) return fail(1, "an attention sink does not support dropout / return_softmax");
    return true;
}

// The fp8 forward's launch (one pass, D = 128): the schedule knobs with fp8_w4 as the kernel
// choice and none of fwd_waves / fwd_prio / fwd_pipe, which its kernels do not read
// The fp8 forward's descales as an entry gives them: by value (the plain entries; the pointers
// null), or device tensors indexed by (batch, kv head) with element strides (the _ex entries)
struct Fp8Descales {
    float q = 1.f, k = 1.f, v = 1.f;
    const float* q_ptr = nullptr; const float* k_ptr = nullptr; const float* v_ptr = nullptr;
    int batch_stride = 0, head_stride = 0;
};
bool check_descales(const Fp8Descales& ds, bool device) {
    if (!device) return (ds.q > 0.f && ds.k > 0.f && ds.v > 0.f) || fail(1, "fp8 descales must be positive");
    if (!ds.q_ptr || !ds.k_ptr || !ds.v_ptr)
        return fail(1, "q_descale, k_descale and v_descale must be non-null device pointers");
    if (ds.batch_stride < 0 || ds.head_stride < 0)
        return fail(1, "descale strides must be non-negative (got %d, %d)", ds.batch_stride, ds.head_stride);
    return true;
}

void run_fwd_fp8(FwdParams& p, const Fp8Descales& ds, int dyn_min,
                 bool out_fp16, hipStream_t st, const char* what) {
    p.q_scale = ds.q; p.k_scale = ds.k; p.v_scale = ds.v;
    p.q_descale = ds.q_ptr; p.k_descale = ds.k_ptr; p.v_descale = ds.v_ptr;
    p.ds_batch = ds.batch_stride; p.ds_head = ds.head_stride;
    load_schedule(p, options().fp8_w4, 8);
    p.num_splits = 1;
    if (!take_item_queue(p, st, dyn_min, 1)) return;
    g_last_splits = 1;
    hip_ok(launch_fwd_fp8(p, out_fp16, st), what);
}

// One knob of XFA_KNOBS by name (nullptr: unknown)
struct Knob { const char* name; std::atomic<int>* slot; int lo, hi; };
const Knob* find_knob(const char* name) {
    Options& o = options();
#define XFA_KNOB_ROW(n, def, lo, hi) {#n, &o.n, lo, hi},
    static const Knob knobs[] = {XFA_KNOBS(XFA_KNOB_ROW)};
#undef XFA_KNOB_ROW
    for (const Knob& k : knobs)
        if (!strcmp(name, k.name)) return &k;
    return nullptr;
}

}  // namespace

extern "C" {

const char* fmha_last_error(void) { return g_err.c_str(); }
int fmha_last_status(void) { return g_status; }
int fmha_last_num_splits(void) { return g_last_splits; }
const char* fmha_last_kernel(void) { return g_last_kernel; }
const char* fmha_version(void) { return XFA_VARIANTS ? "xf-fmha-gfx950 2.13 (variants)" : "xf-fmha-gfx950 2.13"; }

void fmha_set_rng_state(uint64_t seed, uint64_t offset) {
    g_seed = seed;
    g_offset = offset;
    g_seed_ptr = g_offset_ptr = nullptr;
    g_rng_out = nullptr;
}

void fmha_set_rng_state_device(const int64_t* seed_ptr, const int64_t* offset_ptr, uint64_t offset_add,
                               int64_t* rng_out) {
    g_seed_ptr = (seed_ptr && offset_ptr) ? seed_ptr : nullptr;
    g_offset_ptr = g_seed_ptr ? offset_ptr : nullptr;
    g_offset_add = offset_add;
    g_rng_out = rng_out;
}

int fmha_set_option(const char* name, int value) {
    clear_error();
    if (!name) { fail(1, "option name is null"); return -1; }
    Options& o = options();
    const Knob* k = find_knob(name);
    if (!k) { fail(1, "unknown option '%s'", name); return -1; }
    // two knobs take only the ends of their range
    const bool ends_only = k->slot == &o.fwd_waves || k->slot == &o.dec_mr;
    if (value < k->lo || value > k->hi || (ends_only && value != k->lo && value != k->hi)) {
        fail(1, "option %s: value %d out of range [%d, %d]", name, value, k->lo, k->hi);
        return -1;
    }
    if (!XFA_VARIANTS && ((k->slot == &o.fwd_w4 && value == 1) || (k->slot == &o.fp8_w4 && value == 2))) {
        fail(1, "option %s = %d selects a kernel only the variants build has "
                "(lib/variants/libpaged-attention.so, build.py --variants)", name, value);
        return -1;
    }
    k->slot->store(value);
    return 0;
}

int fmha_get_option(const char* name) {
    clear_error();
    if (!name) { fail(1, "option name is null"); return -1; }
    if (const Knob* k = find_knob(name)) return k->slot->load();
    fail(1, "unknown option '%s'", name);
    return -1;
}

void fmha_fwd(void* q_ptr, void* k_ptr, void* v_ptr, void* o_ptr, void* alibi_slopes_ptr,
              const int32_t seqlen_q, const int32_t seqlen_k, const int32_t batch_size,
              const int32_t num_heads, const int32_t num_heads_k, const int32_t head_size,
              const float p_dropout, hipStream_t stream, hipDeviceProp_t* /*dprops*/,
              const float softmax_scale, void* p_ptr, void* softmax_lse_ptr,
              int window_size_left, int window_size_right, const float softcap,
              const bool return_softmax, bool is_fp16, int num_splits) {
    try {
        begin_fwd();
        DevRngScope rng_scope;
        if (!check_common(q_ptr, k_ptr, v_ptr, o_ptr, batch_size, num_heads, num_heads_k, head_size)) return;
        REQUIRE(seqlen_q > 0 && seqlen_k > 0, "seqlen_q/seqlen_k must be positive (%d, %d)", seqlen_q, seqlen_k);
        REQUIRE(!return_softmax || p_dropout > 0.f, "return_softmax is only supported when p_dropout > 0.0");
        REQUIRE(!return_softmax || (p_ptr && softmax_lse_ptr), "return_softmax needs the p and softmax_lse buffers");
        if (!slab_ok("q/o", seqlen_q, (int64_t)num_heads * head_size, 2) ||
            !slab_ok("k/v", seqlen_k, (int64_t)num_heads_k * head_size, 2)) return;
        FwdParams p{};
        fwd_common(p, q_ptr, k_ptr, v_ptr, o_ptr, softmax_lse_ptr, batch_size, num_heads, num_heads_k,
                   head_size, seqlen_q, seqlen_k, window_size_left, window_size_right, softmax_scale,
                   softcap, alibi_slopes_ptr, batch_size > 1 ? num_heads : 0);   // paged_attn.cpp:375
        dense_strides(p, seqlen_q, seqlen_k, num_heads, num_heads_k, head_size);
        if (!set_dropout(p, p_dropout, softcap)) return;
        run_fwd(p, !is_fp16, stream, num_splits);
        if (return_softmax && g_status == 0) run_sdmask(p, p_ptr, !is_fp16, stream);
    } catch (...) {
        fail(9, "internal error in fmha_fwd");
    }
}

}  // extern "C"

namespace {

// fmha_fwd_strided (sink = null) and fmha_fwd_sink
void fwd_strided_entry(const char* entry, void* q, void* k, void* v, void* o, void* alibi_slopes,
                       void* softmax_lse, int32_t seqlen_q, int32_t seqlen_k, int32_t batch_size,
                       int32_t num_heads, int32_t num_heads_k, int32_t head_size, const int64_t* st,
                       float softmax_scale, int window_size_left, int window_size_right,
                       float softcap, bool is_fp16, int num_splits, hipStream_t stream,
                       float p_dropout, void* s_dmask, const float* sink) {
    try {
        begin_fwd();
        DevRngScope rng_scope;
        if (!check_common(q, k, v, o, batch_size, num_heads, num_heads_k, head_size)) return;
        if (!check_sink(sink, alibi_slopes, p_dropout, s_dmask)) return;
        REQUIRE(st != nullptr, "strides must be non-null");
        REQUIRE(seqlen_q > 0 && seqlen_k > 0, "seqlen_q/seqlen_k must be positive (%d, %d)", seqlen_q, seqlen_k);
        for (int i = 0; i < 12; ++i) REQUIRE(st[i] >= 0, "strides must be non-negative");
        {   // (a stride over an extent of 1 is never applied)
            const int ext[12] = {batch_size, seqlen_q, num_heads, batch_size, seqlen_k, num_heads_k,
                                 batch_size, seqlen_k, num_heads_k, batch_size, seqlen_q, num_heads};
            for (int i = 0; i < 12; ++i)
                REQUIRE(ext[i] == 1 || st[i] % 8 == 0,
                        "strides must be multiples of 8 elements (16 bytes): stride %d is %lld", i,
                        (long long)st[i]);
        }
        // one sequence's slab of each tensor, addressed with 32-bit offsets by the kernels
        auto slab = [&](const char* what, int rows, int64_t row, int64_t head, int heads) {
            const int64_t bytes = ((int64_t)(rows - 1) * row + (int64_t)(heads - 1) * head + head_size) * 2;
            if (bytes < kMaxSlabBytes) return true;
            return fail(1, "%s: one sequence spans %lld bytes; this build addresses a sequence with "
                        "32-bit offsets and supports < %lld bytes", what, (long long)bytes,
                        (long long)kMaxSlabBytes);
        };
        if (!slab("q", seqlen_q, st[1], st[2], num_heads) || !slab("k", seqlen_k, st[4], st[5], num_heads_k) ||
            !slab("v", seqlen_k, st[7], st[8], num_heads_k) || !slab("o", seqlen_q, st[10], st[11], num_heads)) return;
        FwdParams p{};
        fwd_common(p, q, k, v, o, softmax_lse, batch_size, num_heads, num_heads_k, head_size,
                   seqlen_q, seqlen_k, window_size_left, window_size_right, softmax_scale, softcap,
                   alibi_slopes, batch_size > 1 ? num_heads : 0, sink);
        p.q_batch = st[0]; p.q_row = st[1]; p.q_head = st[2];
        p.k_batch = st[3]; p.k_row = st[4]; p.k_head = st[5];
        p.v_batch = st[6]; p.v_row = st[7]; p.v_head = st[8];
        p.o_batch = st[9]; p.o_row = st[10]; p.o_head = st[11];
        p.lse_batch = (int64_t)num_heads * seqlen_q; p.lse_head = seqlen_q;
        REQUIRE(!s_dmask || (p_dropout > 0.f && softmax_lse), "s_dmask needs p_dropout > 0 and softmax_lse");
        if (!set_dropout(p, p_dropout, softcap)) return;
        run_fwd(p, !is_fp16, stream, num_splits);
        if (s_dmask && g_status == 0) run_sdmask(p, s_dmask, !is_fp16, stream);
    } catch (...) {
        fail(9, "internal error in %s", entry);
    }
}

void fwd_fp8_entry(const char* entry, void* q, void* k, void* v, void* o, void* softmax_lse,
                   const Fp8Descales& ds, bool device_descales, int32_t seqlen_q, int32_t seqlen_k,
                   int32_t batch_size, int32_t num_heads, int32_t num_heads_k, int32_t head_size,
                   float softmax_scale, int window_size_left, int window_size_right, bool out_fp16,
                   hipStream_t stream) {
    try {
        begin_fwd();
        if (!check_common(q, k, v, o, batch_size, num_heads, num_heads_k, head_size)) return;
        REQUIRE(head_size == 128, "the fp8 forward supports head_size 128 (got %d)", head_size);
        REQUIRE(seqlen_q > 0 && seqlen_k > 0, "seqlen_q/seqlen_k must be positive (%d, %d)", seqlen_q, seqlen_k);
        if (!check_descales(ds, device_descales)) return;
        if (!slab_ok("q", seqlen_q, (int64_t)num_heads * head_size, 1) ||
            !slab_ok("k/v", seqlen_k, (int64_t)num_heads_k * head_size, 1) ||
            !slab_ok("o", seqlen_q, (int64_t)num_heads * head_size, 2)) return;
        FwdParams p{};
        fwd_common(p, q, k, v, o, softmax_lse, batch_size, num_heads, num_heads_k, head_size,
                   seqlen_q, seqlen_k, window_size_left, window_size_right, softmax_scale, 0.f, nullptr, 0);
        dense_strides(p, seqlen_q, seqlen_k, num_heads, num_heads_k, head_size);
        // fwd_dyn = 2: the dynamic per-XCD item queues for the dense fp8 launch too
        run_fwd_fp8(p, ds, 2, out_fp16, stream, "fp8 forward launch");
    } catch (...) {
        fail(9, "internal error in %s", entry);
    }
}

void varlen_fwd_fp8_entry(const char* entry, void* q, void* k, void* v, void* o, void* softmax_lse,
                          void* cu_seqlens_q, void* cu_seqlens_k, void* seqused_k,
                          const Fp8Descales& ds, bool device_descales,
                          int32_t max_seqlen_q, int32_t max_seqlen_k, int32_t total_q,
                          int32_t batch_size, int32_t num_heads, int32_t num_heads_k, int32_t head_size,
                          float softmax_scale, int window_size_left, int window_size_right,
                          bool out_fp16, hipStream_t stream) {
    try {
        begin_fwd();
        if (!check_common(q, k, v, o, batch_size, num_heads, num_heads_k, head_size)) return;
        REQUIRE(cu_seqlens_q && cu_seqlens_k, "cu_seqlens_q and cu_seqlens_k must be given");
        REQUIRE(head_size == 128, "the fp8 forward supports head_size 128 (got %d)", head_size);
        if (!check_descales(ds, device_descales)) return;
        REQUIRE(max_seqlen_q > 0, "max_seqlen_q must be positive (got %d)", max_seqlen_q);
        REQUIRE(max_seqlen_k > 0, "max_seqlen_k must be positive (got %d): nothing to attend to", max_seqlen_k);
        REQUIRE(!softmax_lse || total_q > 0, "total_q must be given to address the LSE");
        if (!slab_ok("q", max_seqlen_q, (int64_t)num_heads * head_size, 1) ||
            !slab_ok("k/v", max_seqlen_k, (int64_t)num_heads_k * head_size, 1) ||
            !slab_ok("o", max_seqlen_q, (int64_t)num_heads * head_size, 2) ||
            (softmax_lse && !slab_ok("softmax_lse", total_q, num_heads, 4))) return;
        FwdParams p{};
        fwd_common(p, q, k, v, o, softmax_lse, batch_size, num_heads, num_heads_k, head_size,
                   max_seqlen_q, max_seqlen_k, window_size_left, window_size_right, softmax_scale, 0.f,
                   nullptr, 0);
        packed_strides(p, num_heads, num_heads_k, head_size, total_q);
        p.cu_seqlens_q = (const int*)cu_seqlens_q;
        p.cu_seqlens_k = (const int*)cu_seqlens_k;
        p.seqused_k = (const int*)seqused_k;
        // ragged items balance from the dynamic item queue (fwd_dyn >= 1, as the bf16 varlen
        // launches); fwd_dyn = 0 keeps the static persistent schedules
        run_fwd_fp8(p, ds, 1, out_fp16, stream, "fp8 varlen forward launch");
    } catch (...) {
        fail(9, "internal error in %s", entry);
    }
}

Fp8Descales descales_by_value(float q, float k, float v) {
    Fp8Descales ds;
    ds.q = q; ds.k = k; ds.v = v;
    return ds;
}
Fp8Descales descales_on_device(const float* q, const float* k, const float* v, int batch_stride, int head_stride) {
    Fp8Descales ds;
    ds.q_ptr = q; ds.k_ptr = k; ds.v_ptr = v;
    ds.batch_stride = batch_stride; ds.head_stride = head_stride;
    return ds;
}

}  // namespace

extern "C" {

void fmha_fwd_fp8(void* q, void* k, void* v, void* o, void* softmax_lse, float q_scale,
                  float k_scale, float v_scale, int32_t seqlen_q, int32_t seqlen_k,
                  int32_t batch_size, int32_t num_heads, int32_t num_heads_k, int32_t head_size,
                  float softmax_scale, int window_size_left, int window_size_right, bool out_fp16,
                  hipStream_t stream) {
    fwd_fp8_entry("fmha_fwd_fp8", q, k, v, o, softmax_lse, descales_by_value(q_scale, k_scale, v_scale),
                  false, seqlen_q, seqlen_k, batch_size, num_heads, num_heads_k, head_size,
                  softmax_scale, window_size_left, window_size_right, out_fp16, stream);
}

void fmha_fwd_fp8_ex(void* q, void* k, void* v, void* o, void* softmax_lse, const float* q_descale,
                     const float* k_descale, const float* v_descale, int32_t descale_batch_stride,
                     int32_t descale_head_stride, int32_t seqlen_q, int32_t seqlen_k,
                     int32_t batch_size, int32_t num_heads, int32_t num_heads_k, int32_t head_size,
                     float softmax_scale, int window_size_left, int window_size_right, bool out_fp16,
                     hipStream_t stream) {
    fwd_fp8_entry("fmha_fwd_fp8_ex", q, k, v, o, softmax_lse,
                  descales_on_device(q_descale, k_descale, v_descale, descale_batch_stride, descale_head_stride),
                  true, seqlen_q, seqlen_k, batch_size, num_heads, num_heads_k, head_size,
                  softmax_scale, window_size_left, window_size_right, out_fp16, stream);
}

void fmha_varlen_fwd_fp8(void* q, void* k, void* v, void* o, void* softmax_lse,
                         void* cu_seqlens_q, void* cu_seqlens_k, void* seqused_k,
                         float q_scale, float k_scale, float v_scale,
                         int32_t max_seqlen_q, int32_t max_seqlen_k, int32_t total_q,
                         int32_t batch_size, int32_t num_heads, int32_t num_heads_k, int32_t head_size,
                         float softmax_scale, int window_size_left, int window_size_right,
                         bool out_fp16, hipStream_t stream) {
    varlen_fwd_fp8_entry("fmha_varlen_fwd_fp8", q, k, v, o, softmax_lse, cu_seqlens_q, cu_seqlens_k,
                         seqused_k, descales_by_value(q_scale, k_scale, v_scale), false, max_seqlen_q,
                         max_seqlen_k, total_q, batch_size, num_heads, num_heads_k, head_size,
                         softmax_scale, window_size_left, window_size_right, out_fp16, stream);
}

void fmha_varlen_fwd_fp8_ex(void* q, void* k, void* v, void* o, void* softmax_lse,
                            void* cu_seqlens_q, void* cu_seqlens_k, void* seqused_k,
                            const float* q_descale, const float* k_descale, const float* v_descale,
                            int32_t descale_batch_stride, int32_t descale_head_stride,
                            int32_t max_seqlen_q, int32_t max_seqlen_k, int32_t total_q,
                            int32_t batch_size, int32_t num_heads, int32_t num_heads_k, int32_t head_size,
                            float softmax_scale, int window_size_left, int window_size_right,
                            bool out_fp16, hipStream_t stream) {
    varlen_fwd_fp8_entry("fmha_varlen_fwd_fp8_ex", q, k, v, o, softmax_lse, cu_seqlens_q, cu_seqlens_k,
                         seqused_k,
                         descales_on_device(q_descale, k_descale, v_descale, descale_batch_stride, descale_head_stride),
                         true, max_seqlen_q, max_seqlen_k, total_q, batch_size, num_heads, num_heads_k,
                         head_size, softmax_scale, window_size_left, window_size_right, out_fp16, stream);
}

void fmha_quantize_fp8(const void* x, void* x8, float* descale, const void* cu_seqlens,
                       int32_t batch_size, int32_t seqlen, int32_t num_heads, int32_t group,
                       int32_t head_size, const int64_t* strides, int32_t granularity, bool is_fp16,
                       hipStream_t stream) {
    try {
        begin_fwd();
        REQUIRE(x && x8 && descale && strides, "x, x8, descale and strides must be non-null pointers");
        REQUIRE(batch_size > 0 && batch_size <= 65535, "batch size must be in [1, 65535] (got %d)", batch_size);
        REQUIRE(seqlen > 0, "seqlen must be positive (got %d)", seqlen);
        REQUIRE(num_heads > 0, "num_heads must be positive (got %d)", num_heads);
        REQUIRE(head_size > 0 && head_size % 8 == 0 && head_size <= 256,
                "head_size must be a multiple of 8 and at most 256 (got %d)", head_size);
        REQUIRE(group > 0 && num_heads % group == 0,
                "group must divide the number of heads (heads=%d, group=%d)", num_heads, group);
        REQUIRE(granularity == 0 || granularity == 1,
                "granularity must be 0 (per tensor) or 1 (per batch and head group), got %d", granularity);
        REQUIRE(!(((uintptr_t)x) & 15) && !(((uintptr_t)x8) & 7),
                "x must be 16-byte and x8 8-byte aligned device pointers");
        const int ext[3] = {cu_seqlens ? 1 : batch_size, seqlen, num_heads};
        for (int i = 0; i < 3; ++i)
            REQUIRE(strides[i] >= 0 && (ext[i] == 1 || strides[i] % 8 == 0),
                    "strides must be non-negative multiples of 8 elements (16 bytes): stride %d is %lld",
                    i, (long long)strides[i]);
        {   // the slab rule of the other entries (one sequence's rows of x)
            const int64_t bytes = ((int64_t)(seqlen - 1) * strides[1] + (int64_t)(num_heads - 1) * strides[2] + head_size) * 2;
            REQUIRE(bytes < kMaxSlabBytes, "x: one sequence spans %lld bytes; this build supports < %lld bytes",
                    (long long)bytes, (long long)kMaxSlabBytes);
        }
        const int nscale = granularity ? batch_size * (num_heads / group) : 1;
        QuantParams p{};
        p.x = x; p.x8 = x8; p.descale = descale; p.cu = (const int*)cu_seqlens;
        p.b = batch_size; p.s = seqlen; p.h = num_heads; p.group = group; p.d = head_size;
        p.gran = granularity;
        p.x_batch = strides[0]; p.x_row = strides[1]; p.x_head = strides[2];
        p.amax = (unsigned*)pool_get(stream, (size_t)nscale * sizeof(unsigned));
        if (!p.amax) { fail(3, "could not allocate the amax accumulator"); return; }
        hip_ok(launch_quantize_fp8(p, is_fp16, stream), "fp8 quantise launch");
    } catch (...) {
        fail(9, "internal error in fmha_quantize_fp8");
    }
}

}  // extern "C"

namespace {

// fmha_varlen_fwd_ex (sink = null) and fmha_varlen_fwd_sink
void varlen_fwd_entry(const char* entry, void* q, void* k, void* v, void* o, void* softmax_lse,
                      void* cu_seqlens_q, void* cu_seqlens_k, void* seqused_k,
                      void* block_table, int32_t block_table_stride, int32_t page_block_size,
                      void* alibi_slopes, int32_t alibi_batch_stride,
                      int32_t max_seqlen_q, int32_t max_seqlen_k, int32_t total_q,
                      int32_t batch_size, int32_t num_heads, int32_t num_heads_k,
                      int32_t head_size, float softmax_scale, int window_size_left,
                      int window_size_right, float softcap, bool is_fp16, hipStream_t stream,
                      float p_dropout, void* s_dmask, const float* sink) {
    try {
        begin_fwd();
        DevRngScope rng_scope;
        if (!check_common(q, k, v, o, batch_size, num_heads, num_heads_k, head_size)) return;
        if (!check_sink(sink, alibi_slopes, p_dropout, s_dmask)) return;
        // (the post-pass walks the packed rows [0, total_q))
        REQUIRE(!sink || total_q > 0, "total_q must be given with a sink");
        REQUIRE(cu_seqlens_q && (cu_seqlens_k || block_table),
                "cu_seqlens_q and cu_seqlens_k (or a block table) must be given");
        REQUIRE(max_seqlen_q > 0 && max_seqlen_k >= 0, "max_seqlen_q must be positive");
        if (max_seqlen_k == 0) { fail(1, "max_seqlen_k == 0: nothing to attend to"); return; }
        if (!slab_ok("q/o", max_seqlen_q, (int64_t)num_heads * head_size, 2) ||
            (!block_table && !slab_ok("k/v", max_seqlen_k, (int64_t)num_heads_k * head_size, 2))) return;
        if (block_table) {
            REQUIRE(page_block_size > 0, "page_block_size must be positive");
            // key lengths from seqused_k or cu_seqlens_k
            REQUIRE(seqused_k || cu_seqlens_k, "paged varlen needs seqused_k or cu_seqlens_k");
        }
        REQUIRE(!softmax_lse || total_q > 0, "total_q must be given to address the LSE");
        REQUIRE(!s_dmask || (p_dropout > 0.f && softmax_lse && !block_table),
                "s_dmask needs p_dropout > 0, softmax_lse and a non-paged K/V");
        REQUIRE(p_dropout == 0.f || !block_table, "dropout over a paged K/V cache is not supported");
        FwdParams p{};
        fwd_common(p, q, k, v, o, softmax_lse, batch_size, num_heads, num_heads_k, head_size,
                   max_seqlen_q, max_seqlen_k, window_size_left, window_size_right, softmax_scale,
                   softcap, alibi_slopes, alibi_batch_stride, sink);
        packed_strides(p, num_heads, num_heads_k, head_size, total_q);
        if (block_table) paged_kv(p, block_table, block_table_stride, page_block_size, num_heads_k, head_size);
        p.cu_seqlens_q = (const int*)cu_seqlens_q;
        p.cu_seqlens_k = (const int*)cu_seqlens_k;
        p.seqused_k = (const int*)seqused_k;
        if (!set_dropout(p, p_dropout, softcap)) return;
        run_fwd(p, !is_fp16, stream, 1);
        if (s_dmask && g_status == 0) run_sdmask(p, s_dmask, !is_fp16, stream);
    } catch (...) {
        fail(9, "internal error in %s", entry);
    }
}

// fmha_page_kvcache_fwd_ex (sink = null) and fmha_page_kvcache_fwd_sink
void page_kvcache_entry(const char* entry, void* q, void* kcache, void* vcache, void* o, void* softmax_lse,
                        void* block_table, int32_t block_table_stride, void* cache_seqlens,
                        int32_t seqlen_q, int32_t max_seqlen_k, int32_t batch_size,
                        int32_t num_heads, int32_t num_heads_k, int32_t head_size,
                        int32_t page_block_size, float softmax_scale,
                        int window_size_left, int window_size_right, float softcap,
                        void* alibi_slopes, int32_t alibi_batch_stride, int32_t num_splits,
                        int32_t kv_dtype, float k_scale, float v_scale,
                        void* cache_leftpad, bool is_fp16, hipStream_t stream, const float* sink) {
    try {
        begin_fwd();
        if (!check_common(q, kcache, vcache, o, batch_size, num_heads, num_heads_k, head_size)) return;
        if (!check_sink(sink, alibi_slopes, 0.f, nullptr)) return;
        REQUIRE(block_table, "block_table must be given for the paged KV path");
        REQUIRE(page_block_size > 0, "page_block_size must be positive");
        REQUIRE(seqlen_q > 0 && max_seqlen_k > 0, "seqlen_q / seqlen_k must be positive");
        REQUIRE(kv_dtype == 0 || kv_dtype == 1, "kv_dtype must be 0 (same as q) or 1 (fp8 e4m3fn)");
        REQUIRE(block_table_stride > 0, "block_table_stride must be positive");
        // export.cpp:1627-1628 (commented out in the reference): no paged KV with leftpad
        REQUIRE(!cache_leftpad || max_seqlen_k <= page_block_size,
                "cache_leftpad needs a non-paged cache (one page per sequence): Paged KV and "
                "leftpad_k are not supported at the same time");
        if (!slab_ok("q/o", seqlen_q, (int64_t)num_heads * head_size, 2) ||
            !slab_ok("kcache/vcache page", page_block_size, (int64_t)num_heads_k * head_size, kv_dtype == 1 ? 1 : 2)) return;
        FwdParams p{};
        fwd_common(p, q, kcache, vcache, o, softmax_lse, batch_size, num_heads, num_heads_k, head_size,
                   seqlen_q, max_seqlen_k, window_size_left, window_size_right, softmax_scale, softcap,
                   alibi_slopes, alibi_batch_stride, sink);
        dense_strides(p, seqlen_q, max_seqlen_k, num_heads, num_heads_k, head_size);
        paged_kv(p, block_table, block_table_stride, page_block_size, num_heads_k, head_size);
        p.seqused_k = (const int*)cache_seqlens;         // non-cumulative (paged_attn.cpp:518-519)
        p.leftpad_k = (const int*)cache_leftpad;
        p.kv_fp8 = kv_dtype == 1; p.k_scale = k_scale; p.v_scale = v_scale;
        run_fwd(p, !is_fp16, stream, num_splits);
    } catch (...) {
        fail(9, "internal error in %s", entry);
    }
}

}  // namespace

extern "C" {

void fmha_fwd_strided(void* q, void* k, void* v, void* o, void* alibi_slopes, void* softmax_lse,
                      int32_t seqlen_q, int32_t seqlen_k, int32_t batch_size, int32_t num_heads,
                      int32_t num_heads_k, int32_t head_size, const int64_t* st,
                      float softmax_scale, int window_size_left, int window_size_right,
                      float softcap, bool is_fp16, int num_splits, hipStream_t stream,
                      float p_dropout, void* s_dmask) {
    fwd_strided_entry("fmha_fwd_strided", q, k, v, o, alibi_slopes, softmax_lse, seqlen_q, seqlen_k,
                      batch_size, num_heads, num_heads_k, head_size, st, softmax_scale,
                      window_size_left, window_size_right, softcap, is_fp16, num_splits, stream,
                      p_dropout, s_dmask, nullptr);
}

void fmha_fwd_sink(void* q, void* k, void* v, void* o, void* alibi_slopes, void* softmax_lse,
                   int32_t seqlen_q, int32_t seqlen_k, int32_t batch_size, int32_t num_heads,
                   int32_t num_heads_k, int32_t head_size, const int64_t* st,
                   float softmax_scale, int window_size_left, int window_size_right,
                   float softcap, bool is_fp16, int num_splits, hipStream_t stream,
                   float p_dropout, void* s_dmask, const float* sink) {
    fwd_strided_entry("fmha_fwd_sink", q, k, v, o, alibi_slopes, softmax_lse, seqlen_q, seqlen_k,
                      batch_size, num_heads, num_heads_k, head_size, st, softmax_scale,
                      window_size_left, window_size_right, softcap, is_fp16, num_splits, stream,
                      p_dropout, s_dmask, sink);
}

void fmha_varlen_fwd_ex(void* q, void* k, void* v, void* o, void* softmax_lse,
                        void* cu_seqlens_q, void* cu_seqlens_k, void* seqused_k,
                        void* block_table, int32_t block_table_stride, int32_t page_block_size,
                        void* alibi_slopes, int32_t alibi_batch_stride,
                        int32_t max_seqlen_q, int32_t max_seqlen_k, int32_t total_q,
                        int32_t batch_size, int32_t num_heads, int32_t num_heads_k,
                        int32_t head_size, float softmax_scale, int window_size_left,
                        int window_size_right, float softcap, bool is_fp16, hipStream_t stream,
                        float p_dropout, void* s_dmask) {
    varlen_fwd_entry("fmha_varlen_fwd_ex", q, k, v, o, softmax_lse, cu_seqlens_q, cu_seqlens_k,
                     seqused_k, block_table, block_table_stride, page_block_size, alibi_slopes,
                     alibi_batch_stride, max_seqlen_q, max_seqlen_k, total_q, batch_size, num_heads,
                     num_heads_k, head_size, softmax_scale, window_size_left, window_size_right,
                     softcap, is_fp16, stream, p_dropout, s_dmask, nullptr);
}

void fmha_varlen_fwd_sink(void* q, void* k, void* v, void* o, void* softmax_lse,
                          void* cu_seqlens_q, void* cu_seqlens_k, void* seqused_k,
                          void* block_table, int32_t block_table_stride, int32_t page_block_size,
                          void* alibi_slopes, int32_t alibi_batch_stride,
                          int32_t max_seqlen_q, int32_t max_seqlen_k, int32_t total_q,
                          int32_t batch_size, int32_t num_heads, int32_t num_heads_k,
                          int32_t head_size, float softmax_scale, int window_size_left,
                          int window_size_right, float softcap, bool is_fp16, hipStream_t stream,
                          float p_dropout, void* s_dmask, const float* sink) {
    varlen_fwd_entry("fmha_varlen_fwd_sink", q, k, v, o, softmax_lse, cu_seqlens_q, cu_seqlens_k,
                     seqused_k, block_table, block_table_stride, page_block_size, alibi_slopes,
                     alibi_batch_stride, max_seqlen_q, max_seqlen_k, total_q, batch_size, num_heads,
                     num_heads_k, head_size, softmax_scale, window_size_left, window_size_right,
                     softcap, is_fp16, stream, p_dropout, s_dmask, sink);
}

void fmha_varlen_fwd(void* q_ptrs, void* k_ptrs, void* v_ptrs, void* o_ptrs,
                     void* cu_seqlens_q_ptrs, void* cu_seqlens_k_ptrs,
                     const int32_t max_seqlen_q, const int32_t max_seqlen_k,
                     const int32_t batch_size, const int32_t num_heads,
                     const int32_t num_heads_k, const int32_t head_size, hipStream_t stream,
                     const float softmax_scale, const bool /*is_causal*/, const bool is_fp16,
                     int window_size_left, int window_size_right) {
    fmha_varlen_fwd_ex(q_ptrs, k_ptrs, v_ptrs, o_ptrs, nullptr, cu_seqlens_q_ptrs,
                       cu_seqlens_k_ptrs, nullptr, nullptr, 0, 0, nullptr, 0, max_seqlen_q,
                       max_seqlen_k, 0, batch_size, num_heads, num_heads_k, head_size,
                       softmax_scale, window_size_left, window_size_right, 0.f, is_fp16, stream,
                       0.f, nullptr);
}

void fmha_page_kvcache_fwd_ex(void* q, void* kcache, void* vcache, void* o, void* softmax_lse,
                              void* block_table, int32_t block_table_stride, void* cache_seqlens,
                              int32_t seqlen_q, int32_t max_seqlen_k, int32_t batch_size,
                              int32_t num_heads, int32_t num_heads_k, int32_t head_size,
                              int32_t page_block_size, float softmax_scale,
                              int window_size_left, int window_size_right, float softcap,
                              void* alibi_slopes, int32_t alibi_batch_stride, int32_t num_splits,
                              int32_t kv_dtype, float k_scale, float v_scale,
                              void* cache_leftpad, bool is_fp16, hipStream_t stream) {
    page_kvcache_entry("fmha_page_kvcache_fwd_ex", q, kcache, vcache, o, softmax_lse, block_table,
                       block_table_stride, cache_seqlens, seqlen_q, max_seqlen_k, batch_size,
                       num_heads, num_heads_k, head_size, page_block_size, softmax_scale,
                       window_size_left, window_size_right, softcap, alibi_slopes,
                       alibi_batch_stride, num_splits, kv_dtype, k_scale, v_scale, cache_leftpad,
                       is_fp16, stream, nullptr);
}

void fmha_page_kvcache_fwd_sink(void* q, void* kcache, void* vcache, void* o, void* softmax_lse,
                                void* block_table, int32_t block_table_stride, void* cache_seqlens,
                                int32_t seqlen_q, int32_t max_seqlen_k, int32_t batch_size,
                                int32_t num_heads, int32_t num_heads_k, int32_t head_size,
                                int32_t page_block_size, float softmax_scale,
                                int window_size_left, int window_size_right, float softcap,
                                void* alibi_slopes, int32_t alibi_batch_stride, int32_t num_splits,
                                int32_t kv_dtype, float k_scale, float v_scale,
                                void* cache_leftpad, bool is_fp16, hipStream_t stream,
                                const float* sink) {
    page_kvcache_entry("fmha_page_kvcache_fwd_sink", q, kcache, vcache, o, softmax_lse, block_table,
                       block_table_stride, cache_seqlens, seqlen_q, max_seqlen_k, batch_size,
                       num_heads, num_heads_k, head_size, page_block_size, softmax_scale,
                       window_size_left, window_size_right, softcap, alibi_slopes,
                       alibi_batch_stride, num_splits, kv_dtype, k_scale, v_scale, cache_leftpad,
                       is_fp16, stream, sink);
}

}  // extern "C"

namespace {

// fmha_kvcache_append (fp8 = false: the caches in q's dtype) and fmha_kvcache_append_fp8 (e4m3fn
// caches with their descales)
void kvcache_append_entry(const char* entry, bool fp8, float k_scale, float v_scale,
                          void* q, void* q_out, void* kcache, void* vcache, const void* knew,
                          const void* vnew, int32_t seqlen_new, const void* block_table,
                          int32_t block_table_stride, int32_t page_block_size,
                          const void* cache_seqlens, void* seqlens_out, const void* rotary_cos,
                          const void* rotary_sin, int32_t rotary_dim, bool is_rotary_interleaved,
                          bool q_rotary_per_token, int32_t batch_size, int32_t seqlen_q,
                          int32_t num_heads, int32_t num_heads_k, int32_t head_size,
                          bool is_fp16, hipStream_t stream) {
    try {
        clear_error();
        // (k_scale > 0 is false for a NaN too)
        REQUIRE(!fp8 || (k_scale > 0.f && v_scale > 0.f && std::isfinite(k_scale) && std::isfinite(v_scale)),
                "fp8 cache descales must be positive");
        REQUIRE(kcache && vcache && block_table && cache_seqlens,
                "kcache, vcache, block_table and cache_seqlens must be given");
        REQUIRE(seqlen_new >= 0, "seqlen_new must be >= 0");
        REQUIRE(seqlen_new == 0 || (knew && vnew), "new K and V must both be given");
        REQUIRE(batch_size > 0 && num_heads > 0 && num_heads_k > 0 && num_heads % num_heads_k == 0,
                "invalid batch / head counts");
        REQUIRE(head_size > 0 && head_size % 8 == 0 && head_size <= 256,
                "head_size must be a multiple of 8 (<= 256) for the append pass");
        REQUIRE(page_block_size > 0, "page_block_size must be positive");
        REQUIRE(block_table_stride > 0, "block_table_stride must be positive");
        // the kernel reads cache_seqlens while writing seqlens_out: in-place is a race
        REQUIRE(seqlens_out != cache_seqlens, "seqlens_out must not alias cache_seqlens");
        REQUIRE(rotary_dim >= 0 && rotary_dim <= head_size && rotary_dim % 16 == 0,
                "Only rotary dimensions divisible by 16 and <= headdim are supported");
        REQUIRE(rotary_dim == 0 || (rotary_cos && rotary_sin && q && q_out),
                "rotary needs cos, sin, q and q_out");
        AppendParams p{};
        p.q = q; p.q_out = q_out; p.kcache = kcache; p.vcache = vcache;
        p.knew = knew; p.vnew = vnew;
        p.block_table = (const int*)block_table; p.bt_stride = block_table_stride;
        p.page = page_block_size;
        p.cache_seqlens = (const int*)cache_seqlens; p.seqlens_out = (int*)seqlens_out;
        p.cos = rotary_cos; p.sin = rotary_sin; p.rdim = rotary_dim;
        p.interleaved = is_rotary_interleaved; p.q_per_token = q_rotary_per_token;
        p.b = batch_size; p.sq = seqlen_q; p.h = num_heads; p.hk = num_heads_k; p.d = head_size;
        p.snew = seqlen_new;
        p.q_head = head_size; p.q_row = (int64_t)num_heads * head_size;
        p.q_batch = (int64_t)seqlen_q * p.q_row;
        p.kn_head = head_size; p.kn_row = (int64_t)num_heads_k * head_size;
        p.kn_batch = (int64_t)seqlen_new * p.kn_row;
        p.head_stride = head_size; p.row_stride = (int64_t)num_heads_k * head_size;
        p.page_stride = (int64_t)page_block_size * p.row_stride;
        p.cache_fp8 = fp8;
        p.k_inv = fp8 ? 1.f / k_scale : 1.f;
        p.v_inv = fp8 ? 1.f / v_scale : 1.f;
        hip_ok(launch_append(p, is_fp16, stream), "append launch");
    } catch (...) {
        fail(9, "internal error in %s", entry);
    }
}

}  // namespace

extern "C" {

void fmha_kvcache_append(void* q, void* q_out, void* kcache, void* vcache, const void* knew,
                         const void* vnew, int32_t seqlen_new, const void* block_table,
                         int32_t block_table_stride, int32_t page_block_size,
                         const void* cache_seqlens, void* seqlens_out, const void* rotary_cos,
                         const void* rotary_sin, int32_t rotary_dim, bool is_rotary_interleaved,
                         bool q_rotary_per_token, int32_t batch_size, int32_t seqlen_q,
                         int32_t num_heads, int32_t num_heads_k, int32_t head_size,
                         bool is_fp16, hipStream_t stream) {
    kvcache_append_entry("fmha_kvcache_append", false, 1.f, 1.f, q, q_out, kcache, vcache, knew, vnew,
                         seqlen_new, block_table, block_table_stride, page_block_size, cache_seqlens,
                         seqlens_out, rotary_cos, rotary_sin, rotary_dim, is_rotary_interleaved,
                         q_rotary_per_token, batch_size, seqlen_q, num_heads, num_heads_k, head_size,
                         is_fp16, stream);
}

void fmha_kvcache_append_fp8(void* q, void* q_out, void* kcache, void* vcache, const void* knew,
                             const void* vnew, int32_t seqlen_new, const void* block_table,
                             int32_t block_table_stride, int32_t page_block_size,
                             const void* cache_seqlens, void* seqlens_out, const void* rotary_cos,
                             const void* rotary_sin, int32_t rotary_dim, bool is_rotary_interleaved,
                             bool q_rotary_per_token, int32_t batch_size, int32_t seqlen_q,
                             int32_t num_heads, int32_t num_heads_k, int32_t head_size,
                             bool is_fp16, hipStream_t stream, float k_scale, float v_scale) {
    kvcache_append_entry("fmha_kvcache_append_fp8", true, k_scale, v_scale, q, q_out, kcache, vcache,
                         knew, vnew, seqlen_new, block_table, block_table_stride, page_block_size,
                         cache_seqlens, seqlens_out, rotary_cos, rotary_sin, rotary_dim,
                         is_rotary_interleaved, q_rotary_per_token, batch_size, seqlen_q, num_heads,
                         num_heads_k, head_size, is_fp16, stream);
}

void fmha_page_kvcache_fwd(void* q_ptr, void* kcache_ptr, void* vcache_ptr, void* /*k_ptr*/,
                           void* /*v_ptr*/, void* o_ptr, void* block_table_ptr,
                           void* cache_seqlens_k_ptr, const int32_t max_cache_seq_k,
                           const int32_t seqlen_q, const int32_t seqlen_k,
                           const int32_t batch_size, const int32_t num_heads,
                           const int32_t num_heads_k, const int32_t head_size,
                           const int32_t page_block_size, hipStream_t stream,
                           const float softmax_scale, int window_size_left,
                           int window_size_right, const int32_t num_splits,
                           void* /*cache_batch_idx_ptr*/, void* /*rotary_cos_ptr*/,
                           void* /*rotary_sin_ptr*/, bool /*is_causal*/,
                           bool /*is_rotary_interleaved*/, bool is_fp16) {
    if (page_block_size <= 0) { begin_fwd(); fail(1, "page_block_size must be positive"); return; }
    fmha_page_kvcache_fwd_ex(q_ptr, kcache_ptr, vcache_ptr, o_ptr, nullptr, block_table_ptr,
                             max_cache_seq_k / page_block_size, cache_seqlens_k_ptr, seqlen_q,
                             seqlen_k, batch_size, num_heads, num_heads_k, head_size,
                             page_block_size, softmax_scale, window_size_left, window_size_right,
                             0.f, nullptr, 0, num_splits, 0, 1.f, 1.f, nullptr, is_fp16, stream);
}


// ------------------------------------------------------------------ backward -----------
// Workspace: fp32 dq_accum [tokens][h][HD] + fp32 D = rowsum(dO*O) [tokens][h].  Deterministic:
// S = min(ceil(CUs / (b * hk)), key blocks) dq_accum slices (the reference's bound,
// export.cpp:1090-1091, counts query heads: here a workgroup covers a kv head's whole GQA group,
// and no workgroup walks more slices than there are 256-key blocks), and at most what
// kDetSliceCap bytes of slices hold; workgroup (bh, s) adds key blocks s, s + S, ... into slice s
// in order.  Any S >= 1 is a valid schedule (bitwise reproducible for a given S), so a run whose
// workspace holds fewer slices than its device would pick uses as many as fit.
static int bwd_block_n_host(int d) { return hd_bucket(d) > 128 ? 128 : 256; }
static size_t bwd_acc_bytes(int64_t tokens, int h, int d) {
    return (((size_t)tokens * h * hd_bucket(d) * sizeof(float)) + 255) / 256 * 256;
}
static size_t bwd_dsum_bytes(int64_t tokens, int h) {
    return (((size_t)tokens * h * sizeof(float)) + 255) / 256 * 256;
}
constexpr size_t kDetSliceCap = (size_t)8 << 30;     // bytes of dQ slices beyond the first
static int bwd_slices(int64_t tokens, int batch, int h, int hk, int d, int seqlen_k, bool det) {
    if (!det) return 1;
    const int units = std::max(1, batch * hk);
    const int nkb = std::max(1, (seqlen_k + bwd_block_n_host(d) - 1) / bwd_block_n_host(d));
    int s = std::min(nkb, (num_cus(current_device()) + units - 1) / units);
    const size_t acc = std::max<size_t>(256, bwd_acc_bytes(tokens, h, d));
    s = (int)std::min<size_t>((size_t)s, 1 + kDetSliceCap / acc);
    return std::max(1, s);
}
// workspace: [dQ slices][D = rowsum(dO O)][lse_fix: the causal-ALiBi LSE in the kernels' form]
static size_t bwd_ws_bytes(int64_t tokens, int h, int d, int slices) {
    return (size_t)slices * bwd_acc_bytes(tokens, h, d) + 2 * bwd_dsum_bytes(tokens, h);
}
// causal ALiBi: softmax_lse (the reference's convention) -> lse_fix in the kernels' own, which
// the backward then reads
static bool bwd_lse_convention(BwdParams& p, hipStream_t st) {
    if (!(p.alibi && p.alibi_causal)) return true;
    LseAlibiParams a = lse_alibi_params(p, -1.f);
    a.dst = p.lse_fix;
    if (!hip_ok(launch_lse_alibi(a, st), "LSE ALiBi pass")) return false;
    p.lse = p.lse_fix;
    return true;
}
// slices a caller's workspace of `bytes` holds (0 if not even one)
static int bwd_slices_fit(int64_t tokens, int h, int d, size_t bytes) {
    const size_t fixed = 2 * bwd_dsum_bytes(tokens, h), acc = std::max<size_t>(1, bwd_acc_bytes(tokens, h, d));
    return bytes < fixed ? 0 : (int)std::min<size_t>((bytes - fixed) / acc, 1 << 20);
}

size_t fmha_bwd_workspace_size(int32_t seqlen_q, int32_t seqlen_k, int32_t batch_size,
                               int32_t num_heads, int32_t num_heads_k, int32_t head_size,
                               bool deterministic) {
    const int64_t tok = (int64_t)batch_size * seqlen_q;
    return bwd_ws_bytes(tok, num_heads, head_size,
                        bwd_slices(tok, batch_size, num_heads, num_heads_k, head_size, seqlen_k, deterministic));
}

size_t fmha_varlen_bwd_workspace_size(int32_t total_q, int32_t max_seqlen_k, int32_t batch_size,
                                      int32_t num_heads, int32_t num_heads_k, int32_t head_size,
                                      bool deterministic) {
    return bwd_ws_bytes(total_q, num_heads, head_size,
                        bwd_slices(total_q, batch_size, num_heads, num_heads_k, head_size, max_seqlen_k, deterministic));
}

// The pre / convert kernels index (token, head, 16-byte chunk) with one 32-bit thread id.
static bool bwd_rows_ok(int64_t tokens, int h, int d) {
    const int64_t threads = tokens * h * (hd_bucket(d) / 8);
    if (threads < (1LL << 31) - 256) return true;
    return fail(1, "backward: %lld (token, head) rows exceed the 32-bit thread index", (long long)(tokens * h));
}

// What both backward entries check alike, after check_common and before their own lengths
static bool bwd_check(const void* dout, const void* lse, const void* dq, const void* dk,
                      const void* dv, float softcap, float p_dropout) {
    if (!(dout && lse && dq && dk && dv)) return fail(1, "dout/softmax_lse/dq/dk/dv must be non-null");
    if (softcap > 0.f && p_dropout > 0.f) return fail(1, "Softcapping does not support dropout for now");
    return true;
}

// The backward of both entries.  `tokens`: the query rows of the whole batch; `packed`: rows of
// all sequences back to back (no batch strides, LSE and accumulator [h, tokens], cu_seqlens
// give the offsets) instead of dense [b, seqlen, ..]; seqlen_q / seqlen_k: the (maximum)
// sequence lengths.
struct BwdTensors { void *dout, *q, *k, *v, *out, *lse, *dq, *dk, *dv, *alibi, *softmax_d; };
static void bwd_run(const BwdTensors& t, int64_t tokens, bool packed, const void* cu_seqlens_q,
                    const void* cu_seqlens_k, int alibi_bstride, int seqlen_q, int seqlen_k, int b,
                    int h, int hk, int d, float p_dropout, float softmax_scale, int wl, int wr,
                    float softcap, bool deterministic, bool is_fp16, hipStream_t stream,
                    void* workspace, size_t workspace_bytes, const char* what) {
    if (!slab_ok("q/out/dout/dq", seqlen_q, (int64_t)h * d, 2) ||
        !slab_ok("k/v/dk/dv", seqlen_k, (int64_t)hk * d, 2) ||
        !slab_ok("dq_accum", seqlen_q, hd_bucket(d), 4) ||
        !bwd_rows_ok(tokens, h, d)) return;
    int slices = bwd_slices(tokens, b, h, hk, d, seqlen_k, deterministic);
    char* ws = (char*)workspace;
    if (ws) {
        const int fit = bwd_slices_fit(tokens, h, d, workspace_bytes);
        REQUIRE(fit >= 1, "workspace too small (%zu < %zu bytes)", workspace_bytes, bwd_ws_bytes(tokens, h, d, 1));
        slices = std::min(slices, fit);
    }
    const size_t need = bwd_ws_bytes(tokens, h, d, slices);
    if (!ws) ws = (char*)pool_get(stream, need);
    REQUIRE(ws, "could not allocate %zu bytes of backward scratch", need);
    const int hd = hd_bucket(d);
    const int64_t rows = packed ? tokens : seqlen_q;      // rows under one head of the LSE / accumulator
    BwdParams p{};
    p.q = t.q; p.k = t.k; p.v = t.v; p.o = t.out; p.dout = t.dout; p.lse = (const float*)t.lse;
    p.dq = t.dq; p.dk = t.dk; p.dv = t.dv;
    p.dq_accum = (float*)ws;
    const size_t acc = bwd_acc_bytes(tokens, h, d);
    p.dsum = t.softmax_d ? (float*)t.softmax_d : (float*)(ws + slices * acc);
    p.lse_fix = (float*)(ws + slices * acc + bwd_dsum_bytes(tokens, h));
    p.dq_slices = deterministic ? slices : 0;   // slices a workgroup walks into
    p.acc_slice = (int64_t)(acc / sizeof(float));
    p.q_row = p.o_row = p.do_row = p.dq_row = (int64_t)h * d;
    p.k_row = p.v_row = p.dk_row = p.dv_row = (int64_t)hk * d;
    p.q_head = p.o_head = p.do_head = p.dq_head = p.k_head = p.v_head = p.dk_head = p.dv_head = d;
    p.q_batch = p.o_batch = p.do_batch = p.dq_batch = packed ? 0 : (int64_t)seqlen_q * h * d;
    p.k_batch = p.v_batch = p.dk_batch = p.dv_batch = packed ? 0 : (int64_t)seqlen_k * hk * d;
    p.lse_head = rows; p.lse_batch = packed ? 0 : (int64_t)h * rows;
    p.acc_row = hd; p.acc_head = rows * hd; p.acc_batch = packed ? 0 : (int64_t)h * rows * hd;
    p.cu_seqlens_q = (const int*)cu_seqlens_q;
    p.cu_seqlens_k = (const int*)cu_seqlens_k;
    p.alibi = (const float*)t.alibi;
    p.alibi_bstride = alibi_bstride;
    p.b = b; p.h = h; p.hk = hk; p.group = h / hk; p.d = d;
    p.seqlen_q = seqlen_q; p.seqlen_k = seqlen_k;
    p.alibi_causal = set_windows(wl, wr, seqlen_k);
    p.wl = wl; p.wr = wr;
    set_scales(p, softmax_scale, softcap);
    p.softcap_on = softcap > 0.f;
    p.scale = softmax_scale;
    p.device = current_device();
    p.order = options().bwd_order.load();
    p.desc = options().bwd_desc.load();
    if (!set_dropout(p, p_dropout, softcap)) return;
    if (!bwd_lse_convention(p, stream)) return;
    hip_ok(dispatch_bwd(p, !is_fp16, stream), what);
}

void fmha_bwd(void* dout, void* q, void* k, void* v, void* out, void* softmax_lse, void* dq,
              void* dk, void* dv, void* alibi_slopes, void* softmax_d, int32_t seqlen_q,
              int32_t seqlen_k, int32_t batch_size, int32_t num_heads, int32_t num_heads_k,
              int32_t head_size, float p_dropout, float softmax_scale, int window_size_left,
              int window_size_right, float softcap, bool deterministic, bool is_fp16,
              hipStream_t stream, void* workspace, size_t workspace_bytes) {
    try {
        clear_error();
        DevRngScope rng_scope;
        if (!check_common(q, k, v, out, batch_size, num_heads, num_heads_k, head_size) ||
            !bwd_check(dout, softmax_lse, dq, dk, dv, softcap, p_dropout)) return;
        REQUIRE(seqlen_q > 0 && seqlen_k > 0, "seqlen_q/seqlen_k must be positive");
        bwd_run({dout, q, k, v, out, softmax_lse, dq, dk, dv, alibi_slopes, softmax_d},
                (int64_t)batch_size * seqlen_q, false, nullptr, nullptr, batch_size > 1 ? num_heads : 0,
                seqlen_q, seqlen_k, batch_size, num_heads, num_heads_k, head_size, p_dropout,
                softmax_scale, window_size_left, window_size_right, softcap, deterministic, is_fp16,
                stream, workspace, workspace_bytes, "backward launch");
    } catch (...) {
        fail(9, "internal error in fmha_bwd");
    }
}

void fmha_varlen_bwd(void* dout, void* q, void* k, void* v, void* out, void* softmax_lse,
                     void* dq, void* dk, void* dv, void* cu_seqlens_q, void* cu_seqlens_k,
                     void* alibi_slopes, int32_t alibi_batch_stride, int32_t max_seqlen_q,
                     int32_t max_seqlen_k, int32_t total_q, int32_t total_k,
                     int32_t batch_size, int32_t num_heads, int32_t num_heads_k,
                     int32_t head_size, float softmax_scale, int window_size_left,
                     int window_size_right, float softcap, bool deterministic, bool is_fp16,
                     hipStream_t stream, void* workspace, size_t workspace_bytes,
                     void* softmax_d, float p_dropout) {
    try {
        clear_error();
        DevRngScope rng_scope;
        if (!check_common(q, k, v, out, batch_size, num_heads, num_heads_k, head_size) ||
            !bwd_check(dout, softmax_lse, dq, dk, dv, softcap, p_dropout)) return;
        REQUIRE(cu_seqlens_q && cu_seqlens_k, "cu_seqlens_q/cu_seqlens_k must be non-null");
        REQUIRE(total_q > 0 && total_k > 0 && max_seqlen_q > 0 && max_seqlen_k > 0,
                "total/max sequence lengths must be positive");
        bwd_run({dout, q, k, v, out, softmax_lse, dq, dk, dv, alibi_slopes, softmax_d}, total_q, true,
                cu_seqlens_q, cu_seqlens_k, alibi_batch_stride, max_seqlen_q, max_seqlen_k, batch_size,
                num_heads, num_heads_k, head_size, p_dropout, softmax_scale, window_size_left,
                window_size_right, softcap, deterministic, is_fp16, stream, workspace, workspace_bytes,
                "varlen backward launch");
    } catch (...) {
        fail(9, "internal error in fmha_varlen_bwd");
    }
}

void fmha_bwd_sink(const float* softmax_lse, const float* softmax_d, const float* sink, float* dsink,
                   int32_t batch, int32_t num_heads, int32_t rows, int64_t batch_stride,
                   int64_t head_stride, hipStream_t stream) {
    try {
        clear_error();
        REQUIRE(softmax_lse && softmax_d && sink && dsink,
                "softmax_lse, softmax_d, sink and dsink must be non-null device pointers");
        REQUIRE(batch > 0 && num_heads > 0 && rows > 0,
                "batch, num_heads and rows must be positive (got %d, %d, %d)", batch, num_heads, rows);
        REQUIRE(batch_stride >= 0 && head_stride >= rows,
                "strides: batch_stride must be non-negative and head_stride at least rows");
        SinkBwdParams p{};
        p.lse = softmax_lse; p.dsum = softmax_d; p.sink = sink; p.dsink = dsink;
        p.b = batch; p.h = num_heads; p.rows = rows;
        p.batch_stride = batch_stride; p.head_stride = head_stride;
        hip_ok(launch_bwd_sink(p, stream), "sink backward launch");
    } catch (...) {
        fail(9, "internal error in fmha_bwd_sink");
    }
}

static_assert(FMHA_MERGE_MAX_PARTS == kMergeMaxParts, "the header's part limit is the kernel's");

void fmha_merge_states(const void* const* o_parts, const float* const* lse_parts, int32_t num_parts,
                       void* o, float* lse, const float* sink, int32_t batch, int32_t rows,
                       int32_t num_heads, int32_t head_size, const int64_t* strides, bool is_fp16,
                       hipStream_t stream) {
    try {
        clear_error();
        REQUIRE(num_parts >= 1 && num_parts <= FMHA_MERGE_MAX_PARTS,
                "num_parts must be in [1, %d] (got %d)", FMHA_MERGE_MAX_PARTS, num_parts);
        REQUIRE(o_parts && lse_parts && o && strides,
                "o_parts, lse_parts, o and strides must be non-null pointers");
        for (int i = 0; i < num_parts; ++i)
            REQUIRE(o_parts[i] && lse_parts[i], "part %d: o and lse must be non-null device pointers", i);
        REQUIRE(batch >= 0 && rows >= 0 && num_heads > 0,
                "batch and rows must be non-negative and num_heads positive (got %d, %d, %d)", batch, rows,
                num_heads);
        REQUIRE(head_size > 0 && head_size % 8 == 0 && head_size <= 256,
                "head_size must be a multiple of 8 and at most 256 (got %d)", head_size);
        if (batch == 0 || rows == 0) return;
        const int ext[3] = {batch, rows, num_heads};
        for (int i = 0; i < 6; ++i)
            REQUIRE(strides[i] >= 0 && (ext[i % 3] == 1 || strides[i] % 8 == 0) &&
                        (i < 3 || ext[i % 3] == 1 || strides[i] > 0),
                    "strides: O strides must be non-negative multiples of 8 elements (16 bytes), the "
                    "output's positive: stride %d is %lld", i, (long long)strides[i]);
        for (int i = 6; i < 10; ++i)
            REQUIRE(strides[i] >= 0 && (i < 8 || ext[i % 2 ? 2 : 0] == 1 || strides[i] > 0),
                    "strides: LSE strides must be non-negative, the output's positive: stride %d is %lld",
                    i, (long long)strides[i]);
        REQUIRE(!(((uintptr_t)o) & 15), "o must be a 16-byte aligned device pointer");
        for (int i = 0; i < num_parts; ++i)
            REQUIRE(!(((uintptr_t)o_parts[i]) & 15), "part %d: o must be a 16-byte aligned device pointer", i);
        // Aliasing, on the byte ranges the strides span (views interleaved in one buffer count as
        // overlapping): the output may be exactly part 0 - same pointer, same strides - and may
        // touch no other part.
        auto o_span = [&](const int64_t* s) {
            return ((int64_t)(batch - 1) * s[0] + (int64_t)(rows - 1) * s[1] + (int64_t)(num_heads - 1) * s[2] + head_size) * 2;
        };
        auto l_span = [&](const int64_t* s) {
            return ((int64_t)(batch - 1) * s[0] + (int64_t)(num_heads - 1) * s[1] + rows) * 4;
        };
        auto overlap = [](const void* a, int64_t na, const void* b, int64_t nb) {
            const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
            return x < y + (uintptr_t)nb && y < x + (uintptr_t)na;
        };
        const bool o_same = strides[0] == strides[3] && strides[1] == strides[4] && strides[2] == strides[5];
        const bool l_same = strides[6] == strides[8] && strides[7] == strides[9];
        for (int i = 0; i < num_parts; ++i) {
            if (overlap(o, o_span(strides + 3), o_parts[i], o_span(strides)))
                REQUIRE(i == 0 && o == o_parts[0] && o_same,
                        "o overlaps part %d: the output may alias part 0 only, exactly (same pointer and strides)", i);
            if (lse && overlap(lse, l_span(strides + 8), lse_parts[i], l_span(strides + 6)))
                REQUIRE(i == 0 && lse == lse_parts[0] && l_same,
                        "lse overlaps part %d: the output may alias part 0 only, exactly (same pointer and strides)", i);
        }
        const int rpb = 256 / (head_size / 8);
        REQUIRE(((int64_t)batch * rows * num_heads + rpb - 1) / rpb <= 0x7fffffffLL,
                "batch * rows * num_heads = %lld is more than one launch covers",
                (long long)batch * rows * num_heads);
        MergeParams p{};
        for (int i = 0; i < num_parts; ++i) { p.o_parts[i] = o_parts[i]; p.lse_parts[i] = lse_parts[i]; }
        p.o = o; p.lse = lse; p.sink = sink;
        p.po_batch = strides[0]; p.po_row = strides[1]; p.po_head = strides[2];
        p.o_batch = strides[3]; p.o_row = strides[4]; p.o_head = strides[5];
        p.pl_batch = strides[6]; p.pl_head = strides[7];
        p.l_batch = strides[8]; p.l_head = strides[9];
        p.n = num_parts; p.b = batch; p.rows = rows; p.h = num_heads; p.d = head_size;
        hip_ok(launch_merge_states(p, is_fp16, stream), "merge launch");
    } catch (...) {
        fail(9, "internal error in fmha_merge_states");
    }
}

}  // extern "C"

namespace {

// The one body of fmha_mla_decode and fmha_mla_decode_fp8: every check, the split rule, the
// scratch and the launch.  fp8: the cache rows are 656 bytes (512 e4m3, 4 fp32 descales, 64
// rotary features of q's type) instead of 576 elements of q's type.
void mla_decode_run(const char* entry, bool fp8, void* q, void* kv_cache, void* o, void* softmax_lse,
                    void* block_table, int32_t block_table_stride, void* cache_seqlens, int32_t seqlen_q,
                    int32_t max_seqlen_k, int32_t batch_size, int32_t num_heads, int32_t head_size,
                    int32_t head_size_v, int32_t page_block_size, const int64_t* strides,
                    float softmax_scale, int window_size_left, int window_size_right,
                    int32_t num_splits, bool is_fp16, hipStream_t stream) {
    try {
        begin_fwd();
        REQUIRE(q && kv_cache && o, "q, kv_cache and o must be non-null device pointers");
        REQUIRE(block_table, "MLA decode reads the latent cache through a block_table: it must be non-null");
        REQUIRE(cache_seqlens, "cache_seqlens must be a non-null device pointer (int32 [batch])");
        REQUIRE(strides, "strides must be a non-null pointer (q then o: batch, row, head)");
        REQUIRE(head_size == 576 && head_size_v == 512,
                "MLA decode supports (head_size, head_size_v) = (576, 512) only (got (%d, %d))", head_size,
                head_size_v);
        REQUIRE(page_block_size > 0 && page_block_size % 16 == 0,
                "page_block_size must be a positive multiple of 16 (got %d)", page_block_size);
        REQUIRE(window_size_left < 0 && (window_size_right < 0 || window_size_right == 0),
                "MLA decode supports the windows (-1, -1) and (-1, 0) (causal) only (got (%d, %d))",
                window_size_left, window_size_right);
        REQUIRE(num_heads >= 1 && seqlen_q >= 1,
                "num_heads and seqlen_q must be at least 1 (got %d, %d)", num_heads, seqlen_q);
        REQUIRE(batch_size >= 0, "batch size must be non-negative (got %d)", batch_size);
        REQUIRE(num_splits <= 128, "num_splits must be at most 128 (got %d)", num_splits);
        REQUIRE(block_table_stride >= 1 && max_seqlen_k >= 0 &&
                    (int64_t)max_seqlen_k <= (int64_t)block_table_stride * page_block_size,
                "max_seqlen_k must lie in [0, block_table_stride * page_block_size] (got %d, table %d x page %d)",
                max_seqlen_k, block_table_stride, page_block_size);
        const int ext[3] = {batch_size, seqlen_q, num_heads};
        for (int i = 0; i < 6; ++i)
            REQUIRE(strides[i] >= 0 && (ext[i % 3] <= 1 || strides[i] % 8 == 0) &&
                        (i < 3 || ext[i % 3] <= 1 || strides[i] > 0),
                    "strides must be non-negative multiples of 8 elements (16 bytes), the output's "
                    "positive: stride %d is %lld", i, (long long)strides[i]);
        REQUIRE(!((((uintptr_t)q) | ((uintptr_t)kv_cache) | ((uintptr_t)o)) & 15),
                "q, kv_cache and o must be 16-byte aligned device pointers");
        REQUIRE(!((((uintptr_t)block_table) | ((uintptr_t)cache_seqlens) | ((uintptr_t)softmax_lse)) & 3),
                "block_table, cache_seqlens and softmax_lse must be 4-byte aligned device pointers");
        if (!slab_ok("kv_cache page", page_block_size, fp8 ? 656 : 576, fp8 ? 1 : 2)) return;
        REQUIRE((int64_t)seqlen_q * num_heads <= 0x7fffffffLL / 16 &&
                    (int64_t)batch_size * 128 * (((int64_t)seqlen_q * num_heads + 15) / 16) <= 0x7fffffffLL,
                "batch_size * seqlen_q * num_heads = %lld is more than one launch covers",
                (long long)batch_size * seqlen_q * num_heads);
        if (batch_size == 0) return;
        MlaParams p{};
        p.q = q; p.kv = kv_cache; p.o = o; p.lse = (float*)softmax_lse;
        p.block_table = (const int*)block_table; p.cache_seqlens = (const int*)cache_seqlens;
        p.q_batch = strides[0]; p.q_row = strides[1]; p.q_head = strides[2];
        p.o_batch = strides[3]; p.o_row = strides[4]; p.o_head = strides[5];
        p.bt_stride = block_table_stride; p.page_size = page_block_size; p.max_seqlen_k = max_seqlen_k;
        p.b = batch_size; p.h = num_heads; p.seqlen_q = seqlen_q;
        p.row_tiles = (seqlen_q * num_heads + 15) / 16;
        p.causal = window_size_right == 0;
        p.scale_log2 = softmax_scale * kLog2e;
        p.device = current_device();
        p.num_cus = num_cus(p.device);
        // Splits: one workgroup (4 waves = 4 items, one per SIMD; its images fill the LDS) per CU
        // over all (batch, row tile, split) items, at most the key tiles and 128
        const int tiles = std::max(1, (max_seqlen_k + 31) / 32);
        int splits = num_splits;
        if (splits <= 0) {
            const int64_t units = (int64_t)batch_size * p.row_tiles;
            splits = (int)std::min<int64_t>(128, (4LL * p.num_cus + units - 1) / units);
        }
        splits = std::max(1, std::min(splits, std::min(tiles, 128)));
        p.num_splits = splits;
        g_last_splits = splits;
        if (splits > 1) {
            const size_t rows = (size_t)batch_size * num_heads * seqlen_q;
            const size_t obytes = (size_t)splits * rows * 512 * sizeof(float);
            const size_t lbytes = (size_t)splits * rows * sizeof(float);
            char* base = (char*)pool_get(stream, obytes + lbytes);
            if (!base) { fail(3, "could not allocate %zu bytes of split scratch", obytes + lbytes); return; }
            p.oaccum = (float*)base;
            p.lseaccum = (float*)(base + obytes);
        }
        hip_ok(fp8 ? launch_mla_decode_fp8(p, is_fp16, stream) : launch_mla_decode(p, is_fp16, stream),
               "MLA decode launch");
    } catch (...) {
        fail(9, "internal error in %s", entry);
    }
}

}  // namespace

extern "C" {

void fmha_mla_decode(void* q, void* kv_cache, void* o, void* softmax_lse, void* block_table,
                     int32_t block_table_stride, void* cache_seqlens, int32_t seqlen_q,
                     int32_t max_seqlen_k, int32_t batch_size, int32_t num_heads, int32_t head_size,
                     int32_t head_size_v, int32_t page_block_size, const int64_t* strides,
                     float softmax_scale, int window_size_left, int window_size_right,
                     int32_t num_splits, bool is_fp16, hipStream_t stream) {
    mla_decode_run("fmha_mla_decode", false, q, kv_cache, o, softmax_lse, block_table, block_table_stride,
                   cache_seqlens, seqlen_q, max_seqlen_k, batch_size, num_heads, head_size, head_size_v,
                   page_block_size, strides, softmax_scale, window_size_left, window_size_right, num_splits,
                   is_fp16, stream);
}

void fmha_mla_decode_fp8(void* q, void* kv_cache8, void* o, void* softmax_lse, void* block_table,
                         int32_t block_table_stride, void* cache_seqlens, int32_t seqlen_q,
                         int32_t max_seqlen_k, int32_t batch_size, int32_t num_heads, int32_t head_size,
                         int32_t head_size_v, int32_t page_block_size, const int64_t* strides,
                         float softmax_scale, int window_size_left, int window_size_right,
                         int32_t num_splits, bool is_fp16, hipStream_t stream) {
    mla_decode_run("fmha_mla_decode_fp8", true, q, kv_cache8, o, softmax_lse, block_table, block_table_stride,
                   cache_seqlens, seqlen_q, max_seqlen_k, batch_size, num_heads, head_size, head_size_v,
                   page_block_size, strides, softmax_scale, window_size_left, window_size_right, num_splits,
                   is_fp16, stream);
}

void fmha_mla_cache_append_fp8(const void* latent, int64_t latent_row_stride, const void* k_pe,
                               int64_t k_pe_row_stride, void* kv_cache8, const void* slot_mapping,
                               int32_t num_tokens, int32_t num_blocks, int32_t page_block_size,
                               bool is_fp16, hipStream_t stream) {
    try {
        clear_error();
        REQUIRE(latent && k_pe && kv_cache8 && slot_mapping,
                "latent, k_pe, kv_cache8 and slot_mapping must be non-null device pointers");
        REQUIRE(num_tokens >= 0 && num_blocks >= 0,
                "num_tokens and num_blocks must be non-negative (got %d, %d)", num_tokens, num_blocks);
        REQUIRE(page_block_size > 0 && page_block_size % 16 == 0,
                "page_block_size must be a positive multiple of 16 (got %d)", page_block_size);
        REQUIRE(latent_row_stride >= 0 && k_pe_row_stride >= 0 && latent_row_stride % 8 == 0 &&
                    k_pe_row_stride % 8 == 0,
                "row strides must be non-negative multiples of 8 elements (16 bytes): got %lld, %lld",
                (long long)latent_row_stride, (long long)k_pe_row_stride);
        REQUIRE(!((((uintptr_t)latent) | ((uintptr_t)k_pe) | ((uintptr_t)kv_cache8)) & 15),
                "latent, k_pe and kv_cache8 must be 16-byte aligned device pointers");
        REQUIRE(!(((uintptr_t)slot_mapping) & 7), "slot_mapping must be an 8-byte aligned device pointer (int64)");
        if (num_tokens == 0) return;
        MlaAppendParams p{};
        p.latent = latent; p.k_pe = k_pe; p.cache = kv_cache8; p.slot = (const int64_t*)slot_mapping;
        p.latent_row = latent_row_stride; p.pe_row = k_pe_row_stride;
        p.slots = (int64_t)num_blocks * page_block_size;
        p.tokens = num_tokens;
        hip_ok(launch_mla_append_fp8(p, is_fp16, stream), "MLA cache append launch");
    } catch (...) {
        fail(9, "internal error in fmha_mla_cache_append_fp8");
    }
}

}  // extern "C"

namespace {

// The one body of fmha_mla_decode_sparse and fmha_mla_decode_sparse_fp8: every check, the split
// rule, the scratch and the launch.  The indices are not read here (no sync): the kernel validates
// every entry against num_blocks * page_block_size.
void mla_sparse_run(const char* entry, bool fp8, void* q, void* kv_cache, void* o, void* softmax_lse,
                    void* indices, int64_t indices_batch_stride, int64_t indices_row_stride, int32_t topk,
                    int32_t seqlen_q, int32_t batch_size, int32_t num_heads, int32_t head_size,
                    int32_t head_size_v, int32_t num_blocks, int32_t page_block_size, const int64_t* strides,
                    float softmax_scale, int32_t num_splits, bool is_fp16, hipStream_t stream) {
    try {
        begin_fwd();
        REQUIRE(q && kv_cache && o, "q, kv_cache and o must be non-null device pointers");
        REQUIRE(indices, "the sparse MLA decode reads its keys through indices: it must be non-null");
        REQUIRE(strides, "strides must be a non-null pointer (q then o: batch, row, head)");
        REQUIRE(head_size == 576 && head_size_v == 512,
                "MLA decode supports (head_size, head_size_v) = (576, 512) only (got (%d, %d))", head_size,
                head_size_v);
        REQUIRE(topk >= 1, "topk must be at least 1 (got %d)", topk);
        REQUIRE(num_blocks >= 1, "num_blocks must be at least 1 (got %d)", num_blocks);
        REQUIRE(page_block_size > 0 && page_block_size % 16 == 0,
                "page_block_size must be a positive multiple of 16 (got %d)", page_block_size);
        REQUIRE(num_heads >= 1 && seqlen_q >= 1,
                "num_heads and seqlen_q must be at least 1 (got %d, %d)", num_heads, seqlen_q);
        REQUIRE(batch_size >= 0, "batch size must be non-negative (got %d)", batch_size);
        REQUIRE(num_splits <= 128, "num_splits must be at most 128 (got %d)", num_splits);
        const int ext[3] = {batch_size, seqlen_q, num_heads};
        for (int i = 0; i < 6; ++i)
            REQUIRE(strides[i] >= 0 && (ext[i % 3] <= 1 || strides[i] % 8 == 0) &&
                        (i < 3 || ext[i % 3] <= 1 || strides[i] > 0),
                    "strides must be non-negative multiples of 8 elements (16 bytes), the output's "
                    "positive: stride %d is %lld", i, (long long)strides[i]);
        REQUIRE(indices_batch_stride >= 0 && indices_row_stride >= 0,
                "the indices strides must be non-negative (got %lld, %lld)",
                (long long)indices_batch_stride, (long long)indices_row_stride);
        REQUIRE(!((((uintptr_t)q) | ((uintptr_t)kv_cache) | ((uintptr_t)o)) & 15),
                "q, kv_cache and o must be 16-byte aligned device pointers");
        REQUIRE(!((((uintptr_t)indices) | ((uintptr_t)softmax_lse)) & 3),
                "indices and softmax_lse must be 4-byte aligned device pointers");
        const int64_t row_tiles = (int64_t)seqlen_q * ((num_heads + 15) / 16);
        REQUIRE((int64_t)seqlen_q * num_heads <= 0x7fffffffLL / 16 &&
                    (int64_t)batch_size * 128 * row_tiles <= 0x7fffffffLL,
                "batch_size * seqlen_q * num_heads = %lld is more than one launch covers",
                (long long)batch_size * seqlen_q * num_heads);
        if (batch_size == 0) return;
        MlaParams p{};
        p.q = q; p.kv = kv_cache; p.o = o; p.lse = (float*)softmax_lse;
        p.indices = (const int*)indices; p.ind_batch = indices_batch_stride; p.ind_row = indices_row_stride;
        p.topk = topk; p.num_slots = (int64_t)num_blocks * page_block_size;
        p.q_batch = strides[0]; p.q_row = strides[1]; p.q_head = strides[2];
        p.o_batch = strides[3]; p.o_row = strides[4]; p.o_head = strides[5];
        p.page_size = page_block_size;
        p.b = batch_size; p.h = num_heads; p.seqlen_q = seqlen_q;
        p.row_tiles = (int)row_tiles;
        p.scale_log2 = softmax_scale * kLog2e;
        p.device = current_device();
        p.num_cus = num_cus(p.device);
        // Splits: fmha_mla_decode's rule over these row tiles, at most the index tiles and 128
        const int tiles = (int)(((int64_t)topk + 31) / 32);
        int splits = num_splits;
        if (splits <= 0) {
            const int64_t units = (int64_t)batch_size * p.row_tiles;
            splits = (int)std::min<int64_t>(128, (4LL * p.num_cus + units - 1) / units);
        }
        splits = std::max(1, std::min(splits, std::min(tiles, 128)));
        p.num_splits = splits;
        g_last_splits = splits;
        if (splits > 1) {
            const size_t rows = (size_t)batch_size * num_heads * seqlen_q;
            const size_t obytes = (size_t)splits * rows * 512 * sizeof(float);
            const size_t lbytes = (size_t)splits * rows * sizeof(float);
            char* base = (char*)pool_get(stream, obytes + lbytes);
            if (!base) { fail(3, "could not allocate %zu bytes of split scratch", obytes + lbytes); return; }
            p.oaccum = (float*)base;
            p.lseaccum = (float*)(base + obytes);
        }
        hip_ok(launch_mla_decode_sparse(p, fp8, is_fp16, stream), "sparse MLA decode launch");
    } catch (...) {
        fail(9, "internal error in %s", entry);
    }
}

}  // namespace

extern "C" {

void fmha_mla_decode_sparse(void* q, void* kv_cache, void* o, void* softmax_lse, void* indices,
                            int64_t indices_batch_stride, int64_t indices_row_stride, int32_t topk,
                            int32_t seqlen_q, int32_t batch_size, int32_t num_heads, int32_t head_size,
                            int32_t head_size_v, int32_t num_blocks, int32_t page_block_size,
                            const int64_t* strides, float softmax_scale, int32_t num_splits, bool is_fp16,
                            hipStream_t stream) {
    mla_sparse_run("fmha_mla_decode_sparse", false, q, kv_cache, o, softmax_lse, indices, indices_batch_stride,
                   indices_row_stride, topk, seqlen_q, batch_size, num_heads, head_size, head_size_v,
                   num_blocks, page_block_size, strides, softmax_scale, num_splits, is_fp16, stream);
}

void fmha_mla_decode_sparse_fp8(void* q, void* kv_cache8, void* o, void* softmax_lse, void* indices,
                                int64_t indices_batch_stride, int64_t indices_row_stride, int32_t topk,
                                int32_t seqlen_q, int32_t batch_size, int32_t num_heads, int32_t head_size,
                                int32_t head_size_v, int32_t num_blocks, int32_t page_block_size,
                                const int64_t* strides, float softmax_scale, int32_t num_splits, bool is_fp16,
                                hipStream_t stream) {
    mla_sparse_run("fmha_mla_decode_sparse_fp8", true, q, kv_cache8, o, softmax_lse, indices,
                   indices_batch_stride, indices_row_stride, topk, seqlen_q, batch_size, num_heads, head_size,
                   head_size_v, num_blocks, page_block_size, strides, softmax_scale, num_splits, is_fp16, stream);
}

}  // extern "C"

namespace {

// ---- MLA prefill: fmha_fwd_mla and fmha_varlen_fwd_mla -------------------------------------
// The pair of head sizes, then the tensors' own strides (q, k, v, o in that order, `per` strides
// each: batch / row / head, or row / head): non-negative, multiples of 8 elements where the
// extent is not 1, K and V rows at least a head apart (a shorter pitch would let the rows past a
// sequence's end alias its own), and one sequence's slab within the 32-bit offsets.
bool check_mla_pair(int head_size_qk, int head_size_v) {
    return (head_size_qk == 192 && head_size_v == 128) ||
           fail(1, "MLA prefill supports (head_size_qk, head_size_v) = (192, 128) only (got (%d, %d))",
                head_size_qk, head_size_v);
}
// (bwd: the backward's eight tensors q, k, v, out, dout, dq, dk, dv - dq goes as q, dk as k, dv
// as v, out and dout as o)
bool check_mla_strides(const int64_t* st, int per, int batch, int rows_q, int rows_k, int h, int hk,
                       bool bwd = false) {
    if (!st) return fail(1, "strides must be non-null");
    static const char* const kFwdName[4] = {"q", "k", "v", "o"};
    static const char* const kBwdName[8] = {"q", "k", "v", "out", "dout", "dq", "dk", "dv"};
    static const int kBwdKind[8] = {0, 1, 2, 3, 3, 0, 1, 2};
    const char* const* kName = bwd ? kBwdName : kFwdName;
    for (int i8 = 0; i8 < (bwd ? 8 : 4); ++i8) {
        const int t = bwd ? kBwdKind[i8] : i8;
        const int rows = (t == 0 || t == 3) ? rows_q : rows_k;
        const int heads = (t == 0 || t == 3) ? h : hk;
        const int width = (t == 0 || t == 1) ? 192 : 128;
        const int64_t* s = st + i8 * per;
        const int64_t row = s[per - 2], head = s[per - 1];
        const int ext[3] = {batch, rows, heads};
        for (int i = 0; i < per; ++i) {
            if (s[i] < 0) return fail(1, "strides must be non-negative: %s stride %d is %lld", kName[i8], i, (long long)s[i]);
            if (ext[3 - per + i] != 1 && s[i] % 8 != 0)
                return fail(1, "strides must be multiples of 8 elements (16 bytes): %s stride %d is %lld",
                            kName[i8], i, (long long)s[i]);
        }
        if ((t == 1 || t == 2) && rows > 1 && row < width)
            return fail(1, "%s row stride must be at least its head size %d (got %lld)", kName[i8], width, (long long)row);
        const int64_t bytes = ((int64_t)(rows - 1) * row + (int64_t)(heads - 1) * head + width) * 2;
        if (bytes >= kMaxSlabBytes)
            return fail(1, "%s: one sequence spans %lld bytes; this build addresses a sequence with "
                        "32-bit offsets and supports < %lld bytes", kName[i8], (long long)bytes,
                        (long long)kMaxSlabBytes);
    }
    return true;
}
// the launch: the schedule knobs every forward shares, one pass, the item queue as run_fwd takes it
// (fwd_dyn >= 1 for packed launches, 2 for dense ones)
void run_fwd_mla(FwdParams& p, bool bf16, hipStream_t st) {
    Options& o = options();
    load_schedule(p, o.fwd_w4, bf16 ? 16 : 15);
    p.prio_hi = o.fwd_prio.load();
    p.pipe = o.fwd_pipe.load();
    p.num_splits = 1;
    g_last_splits = 1;
    if (!take_item_queue(p, st, p.cu_seqlens_q ? 1 : 2, 3)) return;
    hip_ok(bf16 ? launch_fwd_mla_bf16(p, st) : launch_fwd_mla_f16(p, st), "MLA prefill launch");
}

}  // namespace

extern "C" {

void fmha_fwd_mla(void* q, void* k, void* v, void* o, void* softmax_lse, int32_t seqlen_q,
                  int32_t seqlen_k, int32_t batch_size, int32_t num_heads, int32_t num_heads_k,
                  int32_t head_size_qk, int32_t head_size_v, const int64_t* strides,
                  float softmax_scale, int window_size_left, int window_size_right, bool is_fp16,
                  hipStream_t stream) {
    try {
        begin_fwd();
        if (!check_mla_pair(head_size_qk, head_size_v)) return;
        if (!check_common(q, k, v, o, batch_size, num_heads, num_heads_k, head_size_qk)) return;
        REQUIRE(seqlen_q > 0 && seqlen_k > 0, "seqlen_q/seqlen_k must be positive (%d, %d)", seqlen_q, seqlen_k);
        REQUIRE(!(((uintptr_t)softmax_lse) & 3), "softmax_lse must be a 4-byte aligned device pointer");
        if (!check_mla_strides(strides, 3, batch_size, seqlen_q, seqlen_k, num_heads, num_heads_k)) return;
        FwdParams p{};
        fwd_common(p, q, k, v, o, softmax_lse, batch_size, num_heads, num_heads_k, head_size_qk,
                   seqlen_q, seqlen_k, window_size_left, window_size_right, softmax_scale, 0.f, nullptr, 0);
        p.q_batch = strides[0]; p.q_row = strides[1]; p.q_head = strides[2];
        p.k_batch = strides[3]; p.k_row = strides[4]; p.k_head = strides[5];
        p.v_batch = strides[6]; p.v_row = strides[7]; p.v_head = strides[8];
        p.o_batch = strides[9]; p.o_row = strides[10]; p.o_head = strides[11];
        p.lse_batch = (int64_t)num_heads * seqlen_q; p.lse_head = seqlen_q;
        run_fwd_mla(p, !is_fp16, stream);
    } catch (...) {
        fail(9, "internal error in fmha_fwd_mla");
    }
}

void fmha_varlen_fwd_mla(void* q, void* k, void* v, void* o, void* softmax_lse, void* cu_seqlens_q,
                         void* cu_seqlens_k, void* seqused_k, int32_t max_seqlen_q,
                         int32_t max_seqlen_k, int32_t total_q, int32_t batch_size, int32_t num_heads,
                         int32_t num_heads_k, int32_t head_size_qk, int32_t head_size_v,
                         const int64_t* strides, float softmax_scale, int window_size_left,
                         int window_size_right, bool is_fp16, hipStream_t stream) {
    try {
        begin_fwd();
        if (!check_mla_pair(head_size_qk, head_size_v)) return;
        if (!check_common(q, k, v, o, batch_size, num_heads, num_heads_k, head_size_qk)) return;
        REQUIRE(cu_seqlens_q && cu_seqlens_k, "cu_seqlens_q and cu_seqlens_k must be given");
        REQUIRE(max_seqlen_q > 0, "max_seqlen_q must be positive (got %d)", max_seqlen_q);
        REQUIRE(max_seqlen_k > 0, "max_seqlen_k must be positive (got %d): nothing to attend to", max_seqlen_k);
        REQUIRE(!softmax_lse || total_q > 0, "total_q must be given to address the LSE");
        REQUIRE(!(((uintptr_t)softmax_lse | (uintptr_t)cu_seqlens_q | (uintptr_t)cu_seqlens_k | (uintptr_t)seqused_k) & 3),
                "softmax_lse, cu_seqlens_q, cu_seqlens_k and seqused_k must be 4-byte aligned device pointers");
        if (!check_mla_strides(strides, 2, 1, max_seqlen_q, max_seqlen_k, num_heads, num_heads_k)) return;
        if (softmax_lse && !slab_ok("softmax_lse", total_q, num_heads, 4)) return;
        FwdParams p{};
        fwd_common(p, q, k, v, o, softmax_lse, batch_size, num_heads, num_heads_k, head_size_qk,
                   max_seqlen_q, max_seqlen_k, window_size_left, window_size_right, softmax_scale, 0.f,
                   nullptr, 0);
        p.q_row = strides[0]; p.q_head = strides[1];
        p.k_row = strides[2]; p.k_head = strides[3];
        p.v_row = strides[4]; p.v_head = strides[5];
        p.o_row = strides[6]; p.o_head = strides[7];
        p.lse_batch = 0; p.lse_head = total_q;
        p.cu_seqlens_q = (const int*)cu_seqlens_q;
        p.cu_seqlens_k = (const int*)cu_seqlens_k;
        p.seqused_k = (const int*)seqused_k;
        run_fwd_mla(p, !is_fp16, stream);
    } catch (...) {
        fail(9, "internal error in fmha_varlen_fwd_mla");
    }
}

}  // extern "C"

namespace {

// ---- MLA prefill backward: fmha_bwd_mla and fmha_varlen_bwd_mla -----------------------------
// What both entries check alike after the pair and check_common: the backward's own pointers,
// one message an argument
struct MlaBwdTensors { void *dout, *q, *k, *v, *out, *lse, *dq, *dk, *dv, *softmax_d; };
bool check_mla_bwd_ptrs(const MlaBwdTensors& t) {
    const struct { const char* name; const void* ptr; } need[5] = {
        {"dout", t.dout}, {"softmax_lse", t.lse}, {"dq", t.dq}, {"dk", t.dk}, {"dv", t.dv}};
    for (const auto& n : need)
        if (!n.ptr) return fail(1, "%s must be a non-null device pointer", n.name);
    const struct { const char* name; const void* ptr; } vec[4] = {
        {"dout", t.dout}, {"dq", t.dq}, {"dk", t.dk}, {"dv", t.dv}};
    for (const auto& n : vec)
        if ((uintptr_t)n.ptr & 15) return fail(1, "%s must be a 16-byte aligned device pointer", n.name);
    if (((uintptr_t)t.lse | (uintptr_t)t.softmax_d) & 3)
        return fail(1, "softmax_lse and softmax_d must be 4-byte aligned device pointers");
    return true;
}
// The backward of both entries.  `tokens`: the query rows of the whole batch; packed: st holds
// {row, head} of the eight tensors and the LSE / D are [h, tokens], else {batch, row, head} and
// [b, h, seqlen_q].  The only scratch is D (the caller's softmax_d or the stream's pool).
void run_bwd_mla(const MlaBwdTensors& t, const int64_t* st, int64_t tokens, const void* cu_seqlens_q,
                 const void* cu_seqlens_k, int seqlen_q, int seqlen_k, int b, int h, int hk,
                 float softmax_scale, int wl, int wr, bool is_fp16, hipStream_t stream, const char* what) {
    const bool packed = cu_seqlens_q != nullptr;
    // the preprocess kernel indexes (token, head, 16-byte chunk) with one 32-bit thread id
    REQUIRE(tokens * h * 16 < (1LL << 31) - 256,
            "backward: %lld (token, head) rows exceed the 32-bit thread index", (long long)(tokens * h));
    if (!slab_ok("softmax_lse", tokens, h, 4)) return;
    float* dsum = (float*)t.softmax_d;
    if (!dsum) dsum = (float*)pool_get(stream, (size_t)tokens * h * sizeof(float));
    REQUIRE(dsum, "could not allocate %zu bytes of backward scratch", (size_t)tokens * h * sizeof(float));
    BwdParams p{};
    p.q = t.q; p.k = t.k; p.v = t.v; p.o = t.out; p.dout = t.dout; p.lse = (const float*)t.lse;
    p.dq = t.dq; p.dk = t.dk; p.dv = t.dv;
    p.dsum = dsum;
    int64_t* const dst[8][3] = {
        {&p.q_batch, &p.q_row, &p.q_head},    {&p.k_batch, &p.k_row, &p.k_head},
        {&p.v_batch, &p.v_row, &p.v_head},    {&p.o_batch, &p.o_row, &p.o_head},
        {&p.do_batch, &p.do_row, &p.do_head}, {&p.dq_batch, &p.dq_row, &p.dq_head},
        {&p.dk_batch, &p.dk_row, &p.dk_head}, {&p.dv_batch, &p.dv_row, &p.dv_head}};
    const int per = packed ? 2 : 3;
    for (int i = 0; i < 8; ++i) {
        *dst[i][0] = packed ? 0 : st[i * per];
        *dst[i][1] = st[i * per + per - 2];
        *dst[i][2] = st[i * per + per - 1];
    }
    const int64_t rows = packed ? tokens : seqlen_q;      // rows under one head of the LSE / D
    p.lse_head = rows; p.lse_batch = packed ? 0 : (int64_t)h * rows;
    p.cu_seqlens_q = (const int*)cu_seqlens_q;
    p.cu_seqlens_k = (const int*)cu_seqlens_k;
    p.b = b; p.h = h; p.hk = hk; p.group = h / hk; p.d = 192;
    p.seqlen_q = seqlen_q; p.seqlen_k = seqlen_k;
    set_windows(wl, wr, seqlen_k);
    p.wl = wl; p.wr = wr;
    set_scales(p, softmax_scale, 0.f);
    p.scale = softmax_scale;
    p.device = current_device();
    hip_ok(is_fp16 ? launch_bwd_mla_f16(p, tokens, stream) : launch_bwd_mla_bf16(p, tokens, stream), what);
}

}  // namespace

extern "C" {

void fmha_bwd_mla(void* dout, void* q, void* k, void* v, void* out, void* softmax_lse, void* dq,
                  void* dk, void* dv, void* softmax_d, int32_t seqlen_q, int32_t seqlen_k,
                  int32_t batch_size, int32_t num_heads, int32_t num_heads_k, int32_t head_size_qk,
                  int32_t head_size_v, const int64_t* strides, float softmax_scale,
                  int window_size_left, int window_size_right, bool is_fp16, hipStream_t stream) {
    try {
        begin_fwd();
        const MlaBwdTensors t{dout, q, k, v, out, softmax_lse, dq, dk, dv, softmax_d};
        if (!check_mla_pair(head_size_qk, head_size_v)) return;
        if (!check_common(q, k, v, out, batch_size, num_heads, num_heads_k, head_size_qk)) return;
        if (!check_mla_bwd_ptrs(t)) return;
        REQUIRE(seqlen_q > 0 && seqlen_k > 0, "seqlen_q/seqlen_k must be positive (%d, %d)", seqlen_q, seqlen_k);
        if (!check_mla_strides(strides, 3, batch_size, seqlen_q, seqlen_k, num_heads, num_heads_k, true)) return;
        run_bwd_mla(t, strides, (int64_t)batch_size * seqlen_q, nullptr, nullptr, seqlen_q, seqlen_k,
                    batch_size, num_heads, num_heads_k, softmax_scale, window_size_left,
                    window_size_right, is_fp16, stream, "MLA prefill backward launch");
    } catch (...) {
        fail(9, "internal error in fmha_bwd_mla");
    }
}

void fmha_varlen_bwd_mla(void* dout, void* q, void* k, void* v, void* out, void* softmax_lse,
                         void* dq, void* dk, void* dv, void* softmax_d, void* cu_seqlens_q,
                         void* cu_seqlens_k, int32_t max_seqlen_q, int32_t max_seqlen_k,
                         int32_t total_q, int32_t total_k, int32_t batch_size, int32_t num_heads,
                         int32_t num_heads_k, int32_t head_size_qk, int32_t head_size_v,
                         const int64_t* strides, float softmax_scale, int window_size_left,
                         int window_size_right, bool is_fp16, hipStream_t stream) {
    try {
        begin_fwd();
        const MlaBwdTensors t{dout, q, k, v, out, softmax_lse, dq, dk, dv, softmax_d};
        if (!check_mla_pair(head_size_qk, head_size_v)) return;
        if (!check_common(q, k, v, out, batch_size, num_heads, num_heads_k, head_size_qk)) return;
        if (!check_mla_bwd_ptrs(t)) return;
        REQUIRE(cu_seqlens_q && cu_seqlens_k, "cu_seqlens_q and cu_seqlens_k must be given");
        REQUIRE(!(((uintptr_t)cu_seqlens_q | (uintptr_t)cu_seqlens_k) & 3),
                "cu_seqlens_q and cu_seqlens_k must be 4-byte aligned device pointers");
        REQUIRE(max_seqlen_q > 0, "max_seqlen_q must be positive (got %d)", max_seqlen_q);
        REQUIRE(max_seqlen_k > 0, "max_seqlen_k must be positive (got %d): nothing to attend to", max_seqlen_k);
        REQUIRE(total_q > 0 && total_k > 0, "total_q and total_k must be positive (%d, %d)", total_q, total_k);
        if (!check_mla_strides(strides, 2, 1, max_seqlen_q, max_seqlen_k, num_heads, num_heads_k, true)) return;
        run_bwd_mla(t, strides, total_q, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, batch_size,
                    num_heads, num_heads_k, softmax_scale, window_size_left, window_size_right, is_fp16,
                    stream, "MLA prefill varlen backward launch");
    } catch (...) {
        fail(9, "internal error in fmha_varlen_bwd_mla");
    }
}

}  // extern "C"
