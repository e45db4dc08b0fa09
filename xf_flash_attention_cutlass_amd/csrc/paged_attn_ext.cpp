// paged_attn_ext.cpp — the PyTorch op surface: pybind11 module `paged_attn`.
//
// Mirrors the reference's export.cpp (module export.cpp:1757-1764): `fwd` (mha_fwd,
// export.cpp:465-667), `varlen_fwd` (mha_varlen_fwd, :669-937), `fwd_kvcache`
// (mha_fwd_kvcache, :1433-1754) with the same argument lists and return tuples, plus `bwd`
// and `varlen_bwd`, which the reference has only as dead code (:939-1431).  `fwd_kvcache`
// also appends new K/V (with optional rotary) into the cache, which the reference validates
// but never executes (export.cpp:1585-1669, csrc/paged_attn.cpp:513-525).  Every op
// validates with TORCH_CHECK, allocates outputs, and calls the C ABI of
// libpaged-attention.so (include/paged_attn.h); errors reported by the C ABI are re-raised
// as RuntimeError.  Behaviour the reference gets wrong is fixed, not copied:
// LSE is always written; GQA decode is handled by the kernel's head packing instead of the
// transposed-view swap (:526-532); a [H]-shaped ALiBi vector is expanded rather than read
// out of bounds; dropout runs (Philox keep bits, rng_state = {seed, offset} as export.cpp
// returns it) instead of being silently ignored.
//
// Layout: the helpers (one per family of checks), then one function per op.  An op and its
// _sink twin are one function that takes the optional sink first; without_sink / with_sink
// bind the two names to it.
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <c10/core/DeviceGuard.h>
#include <c10/hip/HIPStream.h>
#include <ATen/hip/HIPGeneratorImpl.h>

#include <array>
#include <limits>

#include "paged_attn.h"

#define CHECK_DEVICE(x) TORCH_CHECK(x.is_cuda(), #x " must be on CUDA")
#define CHECK_SHAPE(x, ...) \
    TORCH_CHECK(x.sizes() == torch::IntArrayRef({__VA_ARGS__}), #x " must have shape (" #__VA_ARGS__ ")")
#define CHECK_CONTIGUOUS(x) TORCH_CHECK(x.is_contiguous(), #x " must be contiguous")

namespace {

using OptTensor = c10::optional<at::Tensor>;
using OptConstTensor = c10::optional<const at::Tensor>;

void raise_if_failed(const char* op) {
    if (fmha_last_status() != 0) TORCH_CHECK(false, op, ": ", fmha_last_error());
}

hipStream_t cur_stream() { return c10::hip::getCurrentHIPStream().stream(); }

int round8(int x) { return (x + 7) / 8 * 8; }

void* ptr_or_null(const at::Tensor& t) { return t.defined() ? t.data_ptr() : nullptr; }

at::Tensor pad_last(const at::Tensor& t, int d_og) {
    if (d_og % 8 == 0) return t;
    return torch::nn::functional::pad(t, torch::nn::functional::PadFuncOptions({0, 8 - d_og % 8}));
}

// ... and back: the first d_og columns of a tensor padded to a multiple of 8
at::Tensor unpad_last(const at::Tensor& t, int d_og) {
    if (d_og % 8 == 0) return t;
    return t.index({"...", torch::indexing::Slice(torch::indexing::None, d_og)});
}

// The kernels move 16-byte chunks (b128 buffer loads, LDS-DMA, 16-byte row stores): every base
// pointer must be 16-byte aligned and every row / head / batch stride a multiple of 16 bytes.
bool aligned16(const at::Tensor& t) {
    if ((reinterpret_cast<uintptr_t>(t.data_ptr()) & 15) != 0) return false;
    for (int i = 0; i + 1 < t.dim(); ++i)
        if (t.size(i) > 1 && (t.stride(i) * (int64_t)t.element_size()) % 16 != 0) return false;
    return true;
}

// contiguous AND 16-byte aligned (a view at an odd storage offset is copied)
at::Tensor dense(const at::Tensor& t) {
    at::Tensor c = t.contiguous();
    if (!aligned16(c)) c = c.clone(at::MemoryFormat::Contiguous);
    return c;
}

// ---- rank and shape reading: the rank first (sizes()[i] past it is an unchecked read)
constexpr const char* kDense = "(batch, seqlen, heads, head_size)";
constexpr const char* kPacked = "(total, heads, head_size)";

template <int N>
std::array<int, N> dims(const at::Tensor& t, const char* name, const char* layout) {
    TORCH_CHECK(t.dim() == N, name, " must be ", layout);
    std::array<int, N> s;
    for (int i = 0; i < N; ++i) s[i] = t.size(i);
    return s;
}

void check_qkv_dtype(const at::Tensor& q, const at::Tensor& k, const at::Tensor& v) {
    auto dt = q.dtype();
    TORCH_CHECK(dt == torch::kFloat16 || dt == torch::kBFloat16,
                "FlashAttention only support fp16 and bf16 data type");
    TORCH_CHECK(k.dtype() == dt, "query and key must have the same dtype");
    TORCH_CHECK(v.dtype() == dt, "query and value must have the same dtype");
    CHECK_DEVICE(q); CHECK_DEVICE(k); CHECK_DEVICE(v);
    TORCH_CHECK(q.stride(-1) == 1, "Input tensor must have contiguous last dimension");
    TORCH_CHECK(k.stride(-1) == 1, "Input tensor must have contiguous last dimension");
    TORCH_CHECK(v.stride(-1) == 1, "Input tensor must have contiguous last dimension");
}

// ---- batch, heads and head size (`pass`: "forward" / "backward") ...
void check_heads(int batch_size, int num_heads, int num_heads_k, int head_size, const char* pass) {
    TORCH_CHECK(batch_size > 0, "batch size must be positive");
    TORCH_CHECK(head_size <= 256, "FlashAttention ", pass, " only supports head dimension at most 256");
    TORCH_CHECK(num_heads % num_heads_k == 0, "Number of heads in key/value must divide number of heads in query");
}

// ... and dropout / softcap / return_softmax
void check_dropout(float p_dropout, float softcap, bool return_softmax) {
    TORCH_CHECK(p_dropout >= 0.f && p_dropout < 1.f, "p_dropout must be in [0, 1)");
    if (softcap > 0.f) { TORCH_CHECK(p_dropout == 0.f, "Softcapping does not support dropout for now"); }
    TORCH_CHECK(!return_softmax || p_dropout > 0.f, "return_softmax is only supported when p_dropout > 0.0");
}

// ---- window and causal: causal closes the right window, except for a single query row (which
// sees every key either way; `single_row` is the op's own rule for it); a window that reaches
// past seqlen_k is open.  `fwd` clips before it applies causal (the reference's order,
// export.cpp:497-503), every other op after: with seqlen_k == 0 the first leaves causal's
// right = 0, the second opens it.
void normalize_window(bool is_causal, bool single_row, int seqlen_k, bool clip_first, int& left, int& right) {
    auto clip = [&] {
        if (left >= seqlen_k) left = -1;
        if (right >= seqlen_k) right = -1;
    };
    if (clip_first) clip();
    if (is_causal && !single_row) right = 0;
    if (!clip_first) clip();
}

// ---- cu_seqlens: int32 [batch + 1] on the device, contiguous; returns batch
int check_cu_seqlens(const at::Tensor& cu, const char* name) {
    TORCH_CHECK(cu.dtype() == torch::kInt32, name, " must have dtype int32");
    TORCH_CHECK(cu.is_cuda(), name, " must be on CUDA");
    TORCH_CHECK(cu.is_contiguous(), name, " must be contiguous");
    TORCH_CHECK(cu.dim() == 1 && cu.numel() >= 2, name, " must have shape (batch_size + 1)");
    return cu.numel() - 1;
}
int check_cu_seqlens(const at::Tensor& cu_seqlens_q, const at::Tensor& cu_seqlens_k) {
    const int batch_size = check_cu_seqlens(cu_seqlens_q, "cu_seqlens_q");
    TORCH_CHECK(check_cu_seqlens(cu_seqlens_k, "cu_seqlens_k") == batch_size,
                "cu_seqlens_k must have shape (batch_size + 1)");
    return batch_size;
}

// ---- an int32 [batch] tensor on the device, contiguous: seqused_k, seqlens_k, cache_leftpad
// (leftpad_k), cache_batch_idx; batch_int32 takes an optional one (undefined when absent)
void check_batch_int32(const at::Tensor& t, int batch_size, const char* name) {
    TORCH_CHECK(t.dtype() == torch::kInt32, name, " must have dtype int32");
    TORCH_CHECK(t.is_cuda(), name, " must be on CUDA");
    TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
    TORCH_CHECK(t.dim() == 1 && t.size(0) == batch_size, name, " must have shape (batch_size)");
}
template <typename T>
at::Tensor batch_int32(const c10::optional<T>& t_, int batch_size, const char* name) {
    if (!t_.has_value()) return at::Tensor();
    check_batch_int32(t_.value(), batch_size, name);
    return t_.value();
}

// ---- block_table: int32 [batch, max_num_blocks_per_seq] on the device, rows contiguous
void check_block_table(const at::Tensor& block_table, int batch_size) {
    CHECK_DEVICE(block_table);
    TORCH_CHECK(block_table.dtype() == torch::kInt32, "block_table must have dtype torch.int32");
    TORCH_CHECK(block_table.stride(-1) == 1, "block_table must have contiguous last dimension");
    CHECK_SHAPE(block_table, batch_size, block_table.size(1));
}

// ---- rotary cos / sin [seqlen_ro >= seqlen_k, rotary_dim / 2], q's dtype, contiguous (absent: dim 0)
struct Rotary { at::Tensor cos, sin; int dim = 0; };
template <typename T>
Rotary check_rotary(const c10::optional<T>& cos_, const c10::optional<T>& sin_, const at::Tensor& q,
                    int head_size, int64_t seqlen_k) {
    Rotary r;
    if (!cos_.has_value()) return r;
    TORCH_CHECK(sin_.has_value(), "If rotary cos is provided, rotary sin must also be provided");
    const at::Tensor &cos = cos_.value(), &sin = sin_.value();
    CHECK_DEVICE(cos); CHECK_DEVICE(sin); CHECK_CONTIGUOUS(cos); CHECK_CONTIGUOUS(sin);
    r.dim = cos.size(1) * 2;
    TORCH_CHECK(r.dim <= head_size, "rotary_dim must be <= headdim");
    TORCH_CHECK(r.dim % 16 == 0, "Only rotary dimensions divisible by 16 are currently supported");
    TORCH_CHECK(cos.size(0) >= seqlen_k, "cos/sin seqlen must be at least the seqlen of KV cache");
    CHECK_SHAPE(sin, cos.size(0), r.dim / 2);
    TORCH_CHECK(cos.scalar_type() == q.scalar_type() && sin.scalar_type() == q.scalar_type(),
                "rotary_cos/sin must have the same dtype as query");
    r.cos = cos; r.sin = sin;
    return r;
}

// ---- `out`: the caller's, checked against `shape` (the unpadded one) and `opts`' dtype, when the
// kernel can write it directly: head size a multiple of 8, 16-byte aligned, and contiguous unless
// `strided_ok`.  Otherwise `refuse_indirect` refuses it, or a contiguous temporary of the padded
// shape is computed into and finish_out copies back; the same temporary when no `out` is given.
at::Tensor take_out(const OptTensor& out_, const at::TensorOptions& opts, std::vector<int64_t> shape,
                    bool strided_ok, bool refuse_indirect) {
    if (out_.has_value()) {
        const at::Tensor& out = out_.value();
        TORCH_CHECK(out.dtype() == opts.dtype(), "Output must have the same dtype as inputs");
        CHECK_DEVICE(out);
        TORCH_CHECK(out.stride(-1) == 1, "Output tensor must have contiguous last dimension");
        TORCH_CHECK(out.sizes() == at::IntArrayRef(shape), "out must have shape ", at::IntArrayRef(shape));
        const bool direct = shape.back() % 8 == 0 && aligned16(out) && (strided_ok || out.is_contiguous());
        if (direct) return out;
        TORCH_CHECK(!refuse_indirect, "out must be contiguous (and 16-byte aligned)");
    }
    shape.back() = round8(shape.back());
    return torch::empty(shape, opts);
}

// the op's first result: the padding columns off, and in the caller's `out` when one was given
at::Tensor finish_out(const OptTensor& out_, const at::Tensor& computed, int head_size_og) {
    at::Tensor out = unpad_last(computed, head_size_og);
    if (!out_.has_value() || out_.value().is_same(out)) return out;
    out_.value().copy_(out);
    return out_.value();
}

// ---- gradients (export.cpp:1037-1060): a caller-given tensor must match q/k/v in dtype, device
// and shape; a non-contiguous one is computed into a contiguous temporary and copied back.
// finish_grad returns the caller's view of the result: in its tensor, the padding columns off.
at::Tensor take_grad(const OptTensor& t, const at::Tensor& like) {
    if (t.has_value()) {
        const at::Tensor& x = t.value();
        TORCH_CHECK(x.dtype() == like.dtype(), "gradient must have the same dtype as its input");
        CHECK_DEVICE(x);
        TORCH_CHECK(x.sizes() == like.sizes(), "gradient has the wrong shape");
        if (x.is_contiguous() && aligned16(x)) return x;
    }
    return torch::empty_like(like, like.options().memory_format(at::MemoryFormat::Contiguous));
}
at::Tensor finish_grad(const OptTensor& t, const at::Tensor& g, int head_size_og) {
    if (t.has_value() && !t.value().is_same(g)) t.value().copy_(g);
    return unpad_last(t.has_value() ? t.value() : g, head_size_og);
}

// ALiBi slopes as the C ABI wants them: fp32, [b, h] when batch > 1 (paged_attn.cpp:375).
struct Alibi { at::Tensor slopes; int batch_stride = 0; };
Alibi alibi_for_c(const OptTensor& a, int b, int h) {
    if (!a.has_value()) return {};
    auto s = a.value();
    TORCH_CHECK(s.dtype() == torch::kFloat32, "ALiBi slopes must have dtype fp32");
    CHECK_DEVICE(s);
    TORCH_CHECK(s.stride(-1) == 1, "ALiBi slopes tensor must have contiguous last dimension");
    TORCH_CHECK(s.sizes() == torch::IntArrayRef({h}) || s.sizes() == torch::IntArrayRef({b, h}),
                "ALiBi slopes must have shape (num_heads) or (batch_size, num_heads)");
    if (s.dim() == 1) s = s.unsqueeze(0).expand({b, h});
    return {s.contiguous(), b > 1 ? h : 0};
}

// Dropout: the key from torch's HIP generator (ATen/hip/HIPGeneratorImpl.h, whose generator
// class and Philox state keep their upstream names in this ROCm build: CUDAGeneratorImpl,
// PhiloxCudaState — no other spelling exists) as philox_cuda_state (export.cpp:616-627,
// flash_api_hip.cpp:509): outside stream capture the host seed / offset; under capture the
// generator's device seed / offset pointers, read by the kernels when the graph runs (so every
// replay draws a fresh mask).  rng_state is an int64 [2] on q's device, as upstream returns it;
// the forward kernel writes the key it used into it, and the backward reads it on the device.
at::Tensor dropout_rng(float p_dropout, c10::optional<at::Generator>& gen_, int64_t counter_offset,
                       const at::Device& dev) {
    auto rng = torch::empty({2}, torch::dtype(torch::kInt64).device(dev));
    if (p_dropout > 0.f) {
        auto gen = at::get_generator_or_default<at::CUDAGeneratorImpl>(gen_, at::cuda::detail::getDefaultCUDAGenerator());
        at::PhiloxCudaState st;
        {
            std::lock_guard<std::mutex> lock(gen->mutex_);
            st = gen->philox_cuda_state((uint64_t)counter_offset);
        }
        if (st.captured_) {
            fmha_set_rng_state(0, 0);
            fmha_set_rng_state_device(st.seed_.ptr, st.offset_.ptr, st.offset_intragraph_, rng.data_ptr<int64_t>());
        } else {
            fmha_set_rng_state(st.seed_.val, st.offset_.val);
            fmha_set_rng_state_device(nullptr, nullptr, 0, rng.data_ptr<int64_t>());
        }
    } else {
        fmha_set_rng_state(0, 0);
    }
    return rng;
}

// The backward's key: a device rng_state (the forward's) is read on the device (capturable);
// a host one (a caller's own {seed, offset}) is passed by value.
void dropout_rng_restore(float p_dropout, const OptTensor& rng_state) {
    if (p_dropout <= 0.f) return;
    TORCH_CHECK(rng_state.has_value(), "backward with dropout needs the forward's rng_state");
    const at::Tensor& r0 = rng_state.value();
    TORCH_CHECK(r0.numel() == 2 && r0.scalar_type() == torch::kInt64, "rng_state must be int64 {seed, offset}");
    if (r0.is_cuda()) {
        TORCH_CHECK(r0.is_contiguous(), "rng_state must be contiguous");
        const int64_t* d = r0.data_ptr<int64_t>();
        fmha_set_rng_state(0, 0);
        fmha_set_rng_state_device(d, d + 1, 0, nullptr);
        return;
    }
    auto r = r0.contiguous();
    fmha_set_rng_state((uint64_t)r.data_ptr<int64_t>()[0], (uint64_t)r.data_ptr<int64_t>()[1]);
}

// Disarms the thread's device dropout key when the binding returns or throws: a check
// that fails after dropout_rng / dropout_rng_restore, or a forward with seqlen_k == 0 that runs no
// C entry, must not leave pointers to tensors about to be freed for a later direct C-ABI call.
struct RngDisarm {
    ~RngDisarm() { fmha_set_rng_state_device(nullptr, nullptr, 0, nullptr); }
};

// The sink of the _sink ops: fp32 [num_heads], contiguous, on q's device (null when absent).
const float* sink_for_c(const OptTensor& sink_, const at::Tensor& q, int num_heads) {
    if (!sink_.has_value()) return nullptr;
    const at::Tensor& s = sink_.value();
    TORCH_CHECK(s.dtype() == torch::kFloat32, "sink must have dtype fp32");
    TORCH_CHECK(s.is_cuda() && s.device() == q.device(), "sink must be on q's device");
    TORCH_CHECK(s.dim() == 1 && s.size(0) == num_heads, "sink must have shape (num_heads)");
    CHECK_CONTIGUOUS(s);
    return s.data_ptr<float>();
}

at::Tensor sdmask_buffer(bool want, const at::TensorOptions& opts, int b, int h, int sq, int sk) {
    if (!want) return at::Tensor();
    auto r128 = [](int x) { return (x + 127) / 128 * 128; };
    return torch::empty({b, h, r128(sq), r128(sk)}, opts);
}

// An op and its _sink twin are one function taking the optional sink first: the base name binds
// it without a sink (the reference's argument list; one argument more is a TypeError), the
// _sink name with a trailing, required sink tensor.
template <typename R, typename... A>
auto without_sink(R (*f)(const OptTensor&, A...)) {
    return [f](A... a) { return f(c10::nullopt, std::forward<A>(a)...); };
}
template <typename R, typename... A>
auto with_sink(R (*f)(const OptTensor&, A...)) {
    return [f](A... a, const at::Tensor& sink) { return f(sink, std::forward<A>(a)...); };
}

}  // namespace

// `fwd`, and `fwd_sink` with a trailing sink (fp32 [num_heads])
std::vector<at::Tensor>
mha_fwd(const OptTensor& sink_, at::Tensor& q, const at::Tensor& k, const at::Tensor& v, OptTensor& out_,
        OptTensor& alibi_slopes_, const float p_dropout, const float softmax_scale, bool is_causal,
        int window_size_left, int window_size_right, const float softcap, const bool return_softmax,
        c10::optional<at::Generator> gen_) {
    check_qkv_dtype(q, k, v);
    const auto [batch_size, seqlen_q, num_heads, head_size_og] = dims<4>(q, "q", kDense);
    const int seqlen_k = k.size(1);
    const int num_heads_k = k.size(2);
    check_heads(batch_size, num_heads, num_heads_k, head_size_og, "forward");
    check_dropout(p_dropout, softcap, return_softmax);
    normalize_window(is_causal, seqlen_q == 1 && !alibi_slopes_.has_value(), seqlen_k, /*clip_first=*/true,
                     window_size_left, window_size_right);
    CHECK_SHAPE(k, batch_size, seqlen_k, num_heads_k, head_size_og);
    CHECK_SHAPE(v, batch_size, seqlen_k, num_heads_k, head_size_og);

    // d % 8 == 0 and 16-byte aligned: strided views (head / batch slices, kvpacked kv[:, :, 0])
    // run in place; otherwise the reference's padding to a multiple of 8 (export.cpp:539-547)
    // into aligned contiguous copies.  Either way each tensor goes by its own strides.
    const bool strided = head_size_og % 8 == 0 && aligned16(q) && aligned16(k) && aligned16(v);
    at::Tensor q_padded = strided ? q : dense(pad_last(q, head_size_og));
    at::Tensor k_padded = strided ? k : dense(pad_last(k, head_size_og));
    at::Tensor v_padded = strided ? v : dense(pad_last(v, head_size_og));
    // (an aligned non-contiguous `out` is written in place when the inputs run in place)
    at::Tensor out_padded = take_out(out_, q.options(), {batch_size, seqlen_q, num_heads, head_size_og},
                                     /*strided_ok=*/strided, /*refuse_indirect=*/false);
    const c10::DeviceGuard device_guard(q.device());
    auto opts = q.options();
    auto softmax_lse = torch::empty({batch_size, num_heads, seqlen_q}, opts.dtype(at::kFloat));
    at::Tensor p = sdmask_buffer(return_softmax, opts, batch_size, num_heads, seqlen_q, seqlen_k);
    auto rng_state = dropout_rng(p_dropout, gen_, (int64_t)batch_size * num_heads * 32, q.device());
    RngDisarm rng_disarm;
    const Alibi alibi = alibi_for_c(alibi_slopes_, batch_size, num_heads);
    const float* sink = sink_for_c(sink_, q, num_heads);
    if (seqlen_k > 0) {
        const at::Tensor* t[4] = {&q_padded, &k_padded, &v_padded, &out_padded};
        int64_t st[12];
        for (int i = 0; i < 12; ++i) st[i] = t[i / 3]->stride(i % 3);
        fmha_fwd_sink(q_padded.data_ptr(), k_padded.data_ptr(), v_padded.data_ptr(), out_padded.data_ptr(),
                      ptr_or_null(alibi.slopes), softmax_lse.data_ptr(), seqlen_q, seqlen_k, batch_size,
                      num_heads, num_heads_k, round8(head_size_og), st, softmax_scale, window_size_left,
                      window_size_right, softcap, q.dtype() == torch::kFloat16, 0, cur_stream(), p_dropout,
                      ptr_or_null(p), sink);
        raise_if_failed("fwd");
    } else {
        out_padded.zero_();
        softmax_lse.fill_(std::numeric_limits<float>::infinity());
    }
    return {finish_out(out_, out_padded, head_size_og), q_padded, k_padded, v_padded, out_padded, softmax_lse,
            p, rng_state};
}

// `varlen_fwd`, and `varlen_fwd_sink` with a trailing sink
std::vector<at::Tensor>
mha_varlen_fwd(const OptTensor& sink_, at::Tensor& q, const at::Tensor& k, const at::Tensor& v,
               OptTensor& out_, const at::Tensor& cu_seqlens_q, const at::Tensor& cu_seqlens_k,
               OptTensor& seqused_k, OptTensor& block_table_, OptTensor& alibi_slopes_, int max_seqlen_q,
               const int max_seqlen_k, const float p_dropout, const float softmax_scale,
               const bool zero_tensors, bool is_causal, int window_size_left, int window_size_right,
               const float softcap, const bool return_softmax, c10::optional<at::Generator> gen_) {
    check_qkv_dtype(q, k, v);
    const int batch_size = check_cu_seqlens(cu_seqlens_q, cu_seqlens_k);
    const auto [total_q, num_heads, head_size_og] = dims<3>(q, "q", kPacked);
    at::Tensor block_table;
    const bool paged_KV = block_table_.has_value();
    if (paged_KV) {
        block_table = block_table_.value();
        check_block_table(block_table, batch_size);
    }
    const int num_heads_k = paged_KV ? k.size(2) : k.size(1);
    check_heads(batch_size, num_heads, num_heads_k, head_size_og, "forward");
    check_dropout(p_dropout, softcap, return_softmax);
    TORCH_CHECK(p_dropout == 0.f || !paged_KV, "dropout over a paged K/V cache is not supported");
    const int page_block_size = !paged_KV ? 1 : k.size(1);
    normalize_window(is_causal, max_seqlen_q == 1 && !alibi_slopes_.has_value(), max_seqlen_k,
                     /*clip_first=*/false, window_size_left, window_size_right);
    if (!paged_KV) {
        const int total_k = k.size(0);
        CHECK_SHAPE(k, total_k, num_heads_k, head_size_og);
        CHECK_SHAPE(v, total_k, num_heads_k, head_size_og);
    } else {
        const int num_blocks = k.size(0);
        CHECK_SHAPE(k, num_blocks, page_block_size, num_heads_k, head_size_og);
        CHECK_SHAPE(v, num_blocks, page_block_size, num_heads_k, head_size_og);
    }
    at::Tensor seqused = batch_int32(seqused_k, batch_size, "seqused_k");
    at::Tensor q_padded = dense(pad_last(q, head_size_og));
    at::Tensor k_padded = dense(pad_last(k, head_size_og));
    at::Tensor v_padded = dense(pad_last(v, head_size_og));
    at::Tensor out_padded = take_out(out_, q.options(), {total_q, num_heads, head_size_og},
                                     /*strided_ok=*/false, /*refuse_indirect=*/false);
    const c10::DeviceGuard device_guard(q.device());
    auto opts = q.options();
    auto softmax_lse = torch::empty({num_heads, total_q}, opts.dtype(at::kFloat));
    at::Tensor p = sdmask_buffer(return_softmax, opts, batch_size, num_heads, max_seqlen_q, max_seqlen_k);
    auto rng_state = dropout_rng(p_dropout, gen_, (int64_t)batch_size * num_heads * 32, q.device());
    RngDisarm rng_disarm;
    if (zero_tensors) {
        out_padded.zero_();
        softmax_lse.fill_(-std::numeric_limits<float>::infinity());
    }
    const Alibi alibi = alibi_for_c(alibi_slopes_, batch_size, num_heads);
    const float* sink = sink_for_c(sink_, q, num_heads);
    if (max_seqlen_k > 0) {
        fmha_varlen_fwd_sink(q_padded.data_ptr(), k_padded.data_ptr(), v_padded.data_ptr(),
                             out_padded.data_ptr(), softmax_lse.data_ptr(), cu_seqlens_q.data_ptr(),
                             cu_seqlens_k.data_ptr(), ptr_or_null(seqused), ptr_or_null(block_table),
                             paged_KV ? (int)block_table.stride(0) : 0, page_block_size,
                             ptr_or_null(alibi.slopes), alibi.batch_stride, max_seqlen_q, max_seqlen_k,
                             total_q, batch_size, num_heads, num_heads_k, round8(head_size_og), softmax_scale,
                             window_size_left, window_size_right, softcap, q.dtype() == torch::kFloat16,
                             cur_stream(), p_dropout, ptr_or_null(p), sink);
        raise_if_failed("varlen_fwd");
    } else {
        out_padded.zero_();
        softmax_lse.fill_(std::numeric_limits<float>::infinity());
    }
    return {finish_out(out_, out_padded, head_size_og), q_padded, k_padded, v_padded, out_padded, softmax_lse,
            p, rng_state};
}

// `fwd_kvcache`, and `fwd_kvcache_sink` with a trailing sink
std::vector<at::Tensor>
mha_fwd_kvcache(const OptTensor& sink_, at::Tensor& q, const at::Tensor& kcache, const at::Tensor& vcache,
                OptConstTensor& k_, OptConstTensor& v_, OptConstTensor& seqlens_k_,
                OptConstTensor& rotary_cos_, OptConstTensor& rotary_sin_, OptConstTensor& cache_batch_idx_,
                OptTensor& block_table_, OptTensor& alibi_slopes_, OptTensor& out_, const float softmax_scale,
                bool is_causal, int window_size_left, int window_size_right, const float softcap,
                bool is_rotary_interleaved, int num_splits, OptConstTensor& cache_leftpad_) {
    check_qkv_dtype(q, kcache, vcache);
    const bool append = k_.has_value();
    const bool local_or_causal = is_causal || window_size_left >= 0 || window_size_right >= 0;
    const auto [batch_size, seqlen_q, num_heads, head_size_og] = dims<4>(q, "q", kDense);
    at::Tensor block_table;
    const bool paged_KV = block_table_.has_value();
    if (paged_KV) {
        block_table = block_table_.value();
        check_block_table(block_table, batch_size);
    }
    const int max_num_blocks_per_seq = !paged_KV ? 1 : block_table.size(1);
    const int num_blocks = kcache.size(0);      // (a dense cache: its batch, one "page" per sequence)
    const int page_block_size = kcache.size(1);
    const int seqlen_k = max_num_blocks_per_seq * page_block_size;
    const int num_heads_k = kcache.size(2);
    check_heads(batch_size, num_heads, num_heads_k, head_size_og, "forward");
    normalize_window(is_causal, seqlen_q == 1 && !alibi_slopes_.has_value(), seqlen_k, /*clip_first=*/false,
                     window_size_left, window_size_right);
    CHECK_SHAPE(kcache, num_blocks, page_block_size, num_heads_k, head_size_og);
    CHECK_SHAPE(vcache, num_blocks, page_block_size, num_heads_k, head_size_og);
    if (!paged_KV) {
        // Dense cache [batch_cache, seqlen_k, hk, d] (the reference's non-paged branch dereferences
        // an undefined block_table, export.cpp:1711); the page of batch b is cache_batch_idx[b]
        // when given, else b.
        if (cache_batch_idx_.has_value()) {
            block_table = batch_int32(cache_batch_idx_, batch_size, "cache_batch_idx").view({batch_size, 1});
        } else {
            TORCH_CHECK(num_blocks == batch_size, "k_cache batch must equal q batch without cache_batch_idx");
            block_table = torch::arange(batch_size, q.options().dtype(torch::kInt32)).view({batch_size, 1});
        }
    } else {
        TORCH_CHECK(!cache_batch_idx_.has_value(),
                    "cache_batch_idx cannot be combined with a paged KV cache");
    }
    at::Tensor q_padded = dense(pad_last(q, head_size_og));
    at::Tensor kc = dense(pad_last(kcache, head_size_og));
    at::Tensor vc = dense(pad_last(vcache, head_size_og));
    at::Tensor out = take_out(out_, q.options(), {batch_size, seqlen_q, num_heads, head_size_og},
                              /*strided_ok=*/false, /*refuse_indirect=*/false);
    const int head_size = round8(head_size_og);
    const c10::DeviceGuard device_guard(q.device());
    auto softmax_lse = torch::empty({batch_size, num_heads, seqlen_q}, q.options().dtype(at::kFloat));
    at::Tensor seqlens = batch_int32(seqlens_k_, batch_size, "seqlens_k");
    // cache_leftpad (flash-attn's leftpad_k, commented out at export.cpp:1443,1627-1634): batch b's
    // sequence is cache rows [leftpad[b], seqlens_k[b]); non-paged caches only, as there
    TORCH_CHECK(!cache_leftpad_.has_value() || !paged_KV,
                "We don't support Paged KV and leftpad_k running at the same time yet");
    at::Tensor leftpad = batch_int32(cache_leftpad_, batch_size, "leftpad_k");
    TORCH_CHECK(!leftpad.defined() || seqlens.defined(), "cache_leftpad needs seqlens_k");
    const Alibi alibi = alibi_for_c(alibi_slopes_, batch_size, num_heads);
    const float* sink = sink_for_c(sink_, q, num_heads);
    at::Tensor q_attn = q_padded;
    if (append) {
        // write the new rows into the cache in place (+ rotary on k and q), then attend over the
        // cache with the grown lengths (export.cpp:1585-1669 validation)
        TORCH_CHECK(v_.has_value(), "If key is supplied, value must also be passed in");
        TORCH_CHECK(seqlens.defined(), "If key is supplied, seqlens_k must also be passed in");
        const at::Tensor& kn = k_.value();
        const at::Tensor& vn = v_.value();
        TORCH_CHECK(kn.dtype() == q.dtype(), "Key must have the same dtype as query");
        TORCH_CHECK(vn.dtype() == q.dtype(), "Value must have the same dtype as query");
        CHECK_DEVICE(kn); CHECK_DEVICE(vn); CHECK_CONTIGUOUS(kn); CHECK_CONTIGUOUS(vn);
        const int seqlen_new = kn.size(1);
        CHECK_SHAPE(kn, batch_size, seqlen_new, num_heads_k, head_size_og);
        CHECK_SHAPE(vn, batch_size, seqlen_new, num_heads_k, head_size_og);
        TORCH_CHECK(seqlen_q <= seqlen_k, "If key is supplied, it must have seqlen <= the seqlen of the KV cache");
        TORCH_CHECK(head_size_og % 8 == 0 && kcache.is_contiguous() && vcache.is_contiguous(),
                    "appending needs contiguous caches with head_size a multiple of 8 (updated in place)");
        const Rotary rotary = check_rotary(rotary_cos_, rotary_sin_, q, head_size_og, seqlen_k);
        at::Tensor q_rot = rotary.cos.defined() ? torch::empty_like(q_padded) : at::Tensor();
        auto seqlens_new = torch::empty_like(seqlens);
        fmha_kvcache_append(q_padded.data_ptr(), ptr_or_null(q_rot), kc.data_ptr(), vc.data_ptr(),
                            kn.data_ptr(), vn.data_ptr(), seqlen_new, block_table.data_ptr(),
                            (int)block_table.stride(0), page_block_size, seqlens.data_ptr(),
                            seqlens_new.data_ptr(), ptr_or_null(rotary.cos), ptr_or_null(rotary.sin),
                            rotary.dim, is_rotary_interleaved, local_or_causal, batch_size, seqlen_q,
                            num_heads, num_heads_k, head_size, q.dtype() == torch::kFloat16, cur_stream());
        raise_if_failed("fwd_kvcache (append)");
        seqlens = seqlens_new;
        if (q_rot.defined()) q_attn = q_rot;
    } else {
        TORCH_CHECK(!rotary_cos_.has_value(),
                    "If rotary cos/sin are provided, new key / value to be appended to KV cache must also be provided");
    }
    fmha_page_kvcache_fwd_sink(q_attn.data_ptr(), kc.data_ptr(), vc.data_ptr(), out.data_ptr(),
                               softmax_lse.data_ptr(), block_table.data_ptr(), (int)block_table.stride(0),
                               ptr_or_null(seqlens), seqlen_q, seqlen_k, batch_size, num_heads, num_heads_k,
                               head_size, page_block_size, softmax_scale, window_size_left, window_size_right,
                               softcap, ptr_or_null(alibi.slopes), alibi.batch_stride, num_splits, 0, 1.f, 1.f,
                               ptr_or_null(leftpad), q.dtype() == torch::kFloat16, cur_stream(), sink);
    raise_if_failed("fwd_kvcache");
    return {finish_out(out_, out, head_size_og), softmax_lse};
}

// Gradient of the sink from a backward's saved softmax_lse and its softmax_d: dense
// [batch, heads, seqlen_q] or (varlen) packed [heads, total_q]; returns dsink fp32 [heads].
at::Tensor
mha_sink_bwd(const at::Tensor& softmax_lse, const at::Tensor& softmax_d, const at::Tensor& sink,
             const bool varlen) {
    CHECK_DEVICE(softmax_lse); CHECK_DEVICE(softmax_d); CHECK_DEVICE(sink);
    TORCH_CHECK(softmax_lse.dtype() == torch::kFloat32 && softmax_d.dtype() == torch::kFloat32 &&
                sink.dtype() == torch::kFloat32, "softmax_lse, softmax_d and sink must be fp32");
    TORCH_CHECK(softmax_lse.dim() == (varlen ? 2 : 3), "softmax_lse must be (batch, heads, seqlen_q), or (heads, total_q) with varlen");
    TORCH_CHECK(softmax_d.sizes() == softmax_lse.sizes(), "softmax_d must have softmax_lse's shape");
    CHECK_CONTIGUOUS(softmax_lse); CHECK_CONTIGUOUS(softmax_d); CHECK_CONTIGUOUS(sink);
    const int batch = varlen ? 1 : softmax_lse.size(0);
    const int heads = softmax_lse.size(varlen ? 0 : 1), rows = softmax_lse.size(varlen ? 1 : 2);
    TORCH_CHECK(sink.dim() == 1 && sink.size(0) == heads, "sink must have shape (num_heads)");
    const c10::DeviceGuard device_guard(softmax_lse.device());
    auto dsink = torch::zeros({heads}, sink.options());
    if (batch > 0 && rows > 0) {
        fmha_bwd_sink(softmax_lse.data_ptr<float>(), softmax_d.data_ptr<float>(), sink.data_ptr<float>(),
                      dsink.data_ptr<float>(), batch, heads, rows, (int64_t)heads * rows, rows, cur_stream());
        raise_if_failed("sink_bwd");
    }
    return dsink;
}

namespace {

// ---- `merge_states`: the part lists (count, then every part against part 0) ...
void check_merge_parts(const std::vector<at::Tensor>& parts, size_t count, const char* name, bool lse,
                       int rank, const char* layout) {
    TORCH_CHECK(count >= 1 && count <= FMHA_MERGE_MAX_PARTS, "merge_states takes 1 to ",
                FMHA_MERGE_MAX_PARTS, " parts (got ", count, ")");
    TORCH_CHECK(parts.size() == count, "o_parts and lse_parts must have the same length");
    const at::Tensor& p0 = parts[0];
    if (lse) {
        TORCH_CHECK(p0.dtype() == torch::kFloat32, name, " must have dtype fp32");
    } else {
        TORCH_CHECK(p0.dtype() == torch::kFloat16 || p0.dtype() == torch::kBFloat16, name, " must be fp16 or bf16");
    }
    TORCH_CHECK(p0.dim() == rank, name, " must be ", layout);
    for (const at::Tensor& p : parts) {
        TORCH_CHECK(p.dtype() == p0.dtype(), name, " must share one dtype");
        TORCH_CHECK(p.sizes() == p0.sizes(), name, " must share one shape");
        TORCH_CHECK(p.strides() == p0.strides(), name, " must share one stride set");
    }
    TORCH_CHECK(p0.size(-1) <= 1 || p0.stride(-1) == 1, name, " must have contiguous last dimension");
}

// ... and an output: the caller's (dtype, device and shape of the parts; written in place by its
// own strides) or a new contiguous one
at::Tensor take_merge_out(const OptTensor& t_, const at::Tensor& like, const char* name, bool lse) {
    if (!t_.has_value()) return torch::empty(like.sizes(), like.options());
    const at::Tensor& t = t_.value();
    TORCH_CHECK(t.dtype() == like.dtype(), name, " must have the dtype of the parts");
    TORCH_CHECK(t.is_cuda() && t.device() == like.device(), name, " must be on the parts' device");
    TORCH_CHECK(t.sizes() == like.sizes(), name, " must have the shape of the parts, ", like.sizes());
    TORCH_CHECK(t.size(-1) <= 1 || t.stride(-1) == 1, name, " must have contiguous last dimension");
    if (!lse) { TORCH_CHECK(aligned16(t), name, " must be 16-byte aligned with strides that are multiples of 16 bytes"); }
    return t;
}

}  // namespace

// Merge partial attention states (fmha_merge_states): o_parts dense [batch, rows, heads, d] with
// lse_parts [batch, heads, rows], or packed [total_q, heads, d] with [heads, total_q]; every
// tensor goes by its own strides, nothing is copied.  Returns {out, lse}.
std::vector<at::Tensor>
mha_merge_states(const std::vector<at::Tensor>& o_parts, const std::vector<at::Tensor>& lse_parts,
                 const OptTensor& sink_, const bool packed, const OptTensor& out_, const OptTensor& lse_out_) {
    const size_t n = o_parts.size();
    TORCH_CHECK(lse_parts.size() == n || n < 1 || n > FMHA_MERGE_MAX_PARTS,
                "o_parts and lse_parts must have the same length");
    check_merge_parts(o_parts, n, "o_parts", false, packed ? 3 : 4, packed ? kPacked : kDense);
    check_merge_parts(lse_parts, n, "lse_parts", true, packed ? 2 : 3,
                      packed ? "(heads, total_q)" : "(batch, heads, rows)");
    const at::Tensor& o0 = o_parts[0];
    const at::Tensor& l0 = lse_parts[0];
    const int dim0 = packed ? 0 : 1;
    const int batch = packed ? 1 : o0.size(0), rows = o0.size(dim0), heads = o0.size(dim0 + 1);
    const int head_size = o0.size(dim0 + 2);
    TORCH_CHECK(head_size % 8 == 0 && head_size <= 256, "head_size must be a multiple of 8 and at most 256");
    for (const at::Tensor& p : o_parts)
        TORCH_CHECK(aligned16(p), "o_parts must be 16-byte aligned with strides that are multiples of 16 bytes");
    if (packed) { CHECK_SHAPE(l0, heads, rows); } else { CHECK_SHAPE(l0, batch, heads, rows); }
    for (size_t i = 0; i < n; ++i)
        TORCH_CHECK(o_parts[i].is_cuda() && o_parts[i].device() == o0.device() &&
                    lse_parts[i].device() == o0.device(), "o_parts and lse_parts must be on one CUDA device");
    at::Tensor out = take_merge_out(out_, o0, "out", false);
    at::Tensor lse = take_merge_out(lse_out_, l0, "lse_out", true);
    const float* sink = sink_for_c(sink_, o0, heads);
    if (batch == 0 || rows == 0) return {out, lse};
    const c10::DeviceGuard device_guard(o0.device());
    const void* op[FMHA_MERGE_MAX_PARTS];
    const float* lp[FMHA_MERGE_MAX_PARTS];
    for (size_t i = 0; i < n; ++i) { op[i] = o_parts[i].data_ptr(); lp[i] = lse_parts[i].data_ptr<float>(); }
    const int64_t st[10] = {packed ? 0 : o0.stride(0), o0.stride(dim0), o0.stride(dim0 + 1),
                            packed ? 0 : out.stride(0), out.stride(dim0), out.stride(dim0 + 1),
                            packed ? 0 : l0.stride(0), l0.stride(packed ? 0 : 1),
                            packed ? 0 : lse.stride(0), lse.stride(packed ? 0 : 1)};
    fmha_merge_states(op, lp, (int)n, out.data_ptr(), lse.data_ptr<float>(), sink, batch, rows, heads,
                      head_size, st, o0.dtype() == torch::kFloat16, cur_stream());
    raise_if_failed("merge_states");
    return {out, lse};
}

namespace {

// what `bwd` and `varlen_bwd` check alike before their shapes: q / k / v are the forward's padded
// tensors (head_size), dout the caller's (head_size_og)
void check_bwd_args(const at::Tensor& q, const at::Tensor& k, const at::Tensor& v, float p_dropout,
                    float softcap, const OptTensor& rng_state) {
    check_qkv_dtype(q, k, v);
    check_dropout(p_dropout, softcap, /*return_softmax=*/false);
    dropout_rng_restore(p_dropout, rng_state);
}
void check_bwd_heads(int batch_size, int num_heads, int num_heads_k, int head_size, int head_size_og) {
    TORCH_CHECK(head_size % 8 == 0, "head_size should be a multiple of 8");
    check_heads(batch_size, num_heads, num_heads_k, head_size, "backward");
    TORCH_CHECK(head_size == round8(head_size_og), "head_size must be head_size_og rounded to a multiple of 8");
}

}  // namespace

std::vector<at::Tensor>
mha_bwd(const at::Tensor& dout, const at::Tensor& q, const at::Tensor& k, const at::Tensor& v,
        const at::Tensor& out, const at::Tensor& softmax_lse, OptTensor& dq_, OptTensor& dk_, OptTensor& dv_,
        OptTensor& alibi_slopes_, const float p_dropout, const float softmax_scale, const bool is_causal,
        int window_size_left, int window_size_right, const float softcap, const bool deterministic,
        c10::optional<at::Generator> /*gen_*/, OptTensor& rng_state) {
    TORCH_CHECK(out.dtype() == q.dtype(), "query and out must have the same dtype");
    TORCH_CHECK(dout.dtype() == q.dtype(), "query and dout must have the same dtype");
    CHECK_DEVICE(out); CHECK_DEVICE(dout); CHECK_DEVICE(softmax_lse);
    check_bwd_args(q, k, v, p_dropout, softcap, rng_state);
    RngDisarm rng_disarm;
    const auto [batch_size, seqlen_q, num_heads, head_size] = dims<4>(q, "q", kDense);
    const int head_size_og = dout.size(3);
    const int seqlen_k = k.size(1);
    const int num_heads_k = k.size(2);
    check_bwd_heads(batch_size, num_heads, num_heads_k, head_size, head_size_og);
    normalize_window(is_causal, /*single_row=*/false, seqlen_k, /*clip_first=*/false, window_size_left,
                     window_size_right);
    CHECK_SHAPE(k, batch_size, seqlen_k, num_heads_k, head_size);
    CHECK_SHAPE(v, batch_size, seqlen_k, num_heads_k, head_size);
    CHECK_SHAPE(out, batch_size, seqlen_q, num_heads, head_size);
    CHECK_SHAPE(dout, batch_size, seqlen_q, num_heads, head_size_og);
    CHECK_SHAPE(softmax_lse, batch_size, num_heads, seqlen_q);
    at::Tensor dq = take_grad(dq_, q), dk = take_grad(dk_, k), dv = take_grad(dv_, v);
    at::Tensor dout_padded = dense(pad_last(dout, head_size_og));
    const c10::DeviceGuard device_guard(q.device());
    auto opts = q.options();
    auto softmax_d = torch::empty({batch_size, num_heads, seqlen_q}, opts.dtype(at::kFloat));
    const Alibi alibi = alibi_for_c(alibi_slopes_, batch_size, num_heads);
    auto qc = dense(q), kc = dense(k), vc = dense(v), oc = dense(out);
    auto lse = softmax_lse.contiguous();
    const size_t ws = fmha_bwd_workspace_size(seqlen_q, seqlen_k, batch_size, num_heads, num_heads_k,
                                              head_size, deterministic);
    at::Tensor workspace = torch::empty({(int64_t)ws}, opts.dtype(torch::kUInt8));
    if (seqlen_q > 0) {
        fmha_bwd(dout_padded.data_ptr(), qc.data_ptr(), kc.data_ptr(), vc.data_ptr(), oc.data_ptr(),
                 lse.data_ptr(), dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), ptr_or_null(alibi.slopes),
                 softmax_d.data_ptr(), seqlen_q, seqlen_k, batch_size, num_heads, num_heads_k, head_size,
                 p_dropout, softmax_scale, window_size_left, window_size_right, softcap, deterministic,
                 q.dtype() == torch::kFloat16, cur_stream(), workspace.data_ptr(), ws);
        raise_if_failed("bwd");
    } else {
        dk.zero_(); dv.zero_(); softmax_d.zero_();
    }
    return {finish_grad(dq_, dq, head_size_og), finish_grad(dk_, dk, head_size_og),
            finish_grad(dv_, dv, head_size_og), softmax_d};
}

std::vector<at::Tensor>
mha_varlen_bwd(const at::Tensor& dout, const at::Tensor& q, const at::Tensor& k, const at::Tensor& v,
               const at::Tensor& out, const at::Tensor& softmax_lse, OptTensor& dq_, OptTensor& dk_,
               OptTensor& dv_, const at::Tensor& cu_seqlens_q, const at::Tensor& cu_seqlens_k,
               OptTensor& alibi_slopes_, const int max_seqlen_q, const int max_seqlen_k, const float p_dropout,
               const float softmax_scale, const bool /*zero_tensors*/, const bool is_causal,
               int window_size_left, int window_size_right, const float softcap, const bool deterministic,
               c10::optional<at::Generator> /*gen_*/, OptTensor& rng_state) {
    check_bwd_args(q, k, v, p_dropout, softcap, rng_state);
    RngDisarm rng_disarm;
    const int batch_size = check_cu_seqlens(cu_seqlens_q, cu_seqlens_k);
    const int total_q = q.size(0), num_heads = q.size(1), head_size = q.size(2);
    const int total_k = k.size(0), num_heads_k = k.size(1);
    const int head_size_og = dout.size(2);
    check_bwd_heads(batch_size, num_heads, num_heads_k, head_size, head_size_og);
    normalize_window(is_causal, /*single_row=*/false, max_seqlen_k, /*clip_first=*/false, window_size_left,
                     window_size_right);
    CHECK_SHAPE(softmax_lse, num_heads, total_q);
    CHECK_SHAPE(k, total_k, num_heads_k, head_size);
    CHECK_SHAPE(v, total_k, num_heads_k, head_size);
    CHECK_SHAPE(out, total_q, num_heads, head_size);
    CHECK_SHAPE(dout, total_q, num_heads, head_size_og);
    at::Tensor dq = take_grad(dq_, q), dk = take_grad(dk_, k), dv = take_grad(dv_, v);
    at::Tensor dout_padded = dense(pad_last(dout, head_size_og));
    const c10::DeviceGuard device_guard(q.device());
    auto opts = q.options();
    auto softmax_d = torch::empty({num_heads, total_q}, opts.dtype(at::kFloat));
    const Alibi alibi = alibi_for_c(alibi_slopes_, batch_size, num_heads);
    auto qc = dense(q), kc = dense(k), vc = dense(v), oc = dense(out);
    auto lse = softmax_lse.contiguous();
    const size_t ws = fmha_varlen_bwd_workspace_size(total_q, max_seqlen_k, batch_size, num_heads,
                                                     num_heads_k, head_size, deterministic);
    at::Tensor workspace = torch::empty({(int64_t)ws}, opts.dtype(torch::kUInt8));
    fmha_varlen_bwd(dout_padded.data_ptr(), qc.data_ptr(), kc.data_ptr(), vc.data_ptr(), oc.data_ptr(),
                    lse.data_ptr(), dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), cu_seqlens_q.data_ptr(),
                    cu_seqlens_k.data_ptr(), ptr_or_null(alibi.slopes), alibi.batch_stride, max_seqlen_q,
                    max_seqlen_k, total_q, total_k, batch_size, num_heads, num_heads_k, head_size,
                    softmax_scale, window_size_left, window_size_right, softcap, deterministic,
                    q.dtype() == torch::kFloat16, cur_stream(), workspace.data_ptr(), ws,
                    softmax_d.data_ptr(), p_dropout);
    raise_if_failed("varlen_bwd");
    return {finish_grad(dq_, dq, head_size_og), finish_grad(dk_, dk, head_size_og),
            finish_grad(dv_, dv, head_size_og), softmax_d};
}

// Paged decode over an fp8 (OCP e4m3fn) K/V cache with per-tensor dequant scales — an
// extension the reference lacks.  kcache/vcache: float8_e4m3fn (or uint8 bytes)
// [num_blocks, page, hk, d]; returns {out, softmax_lse}.  `fwd_kvcache_fp8`, and
// `fwd_kvcache_fp8_sink` with a trailing sink.
std::vector<at::Tensor>
mha_fwd_kvcache_fp8(const OptTensor& sink_, at::Tensor& q, const at::Tensor& kcache, const at::Tensor& vcache,
                    const at::Tensor& seqlens_k, const at::Tensor& block_table, const float k_scale,
                    const float v_scale, const float softmax_scale, bool is_causal, int window_size_left,
                    int window_size_right, int num_splits) {
    auto dt = q.dtype();
    TORCH_CHECK(dt == torch::kFloat16 || dt == torch::kBFloat16, "q must be fp16 or bf16");
    TORCH_CHECK(kcache.element_size() == 1 && vcache.element_size() == 1, "fp8 K/V cache expected");
    CHECK_DEVICE(q); CHECK_DEVICE(kcache); CHECK_DEVICE(vcache);
    CHECK_CONTIGUOUS(kcache); CHECK_CONTIGUOUS(vcache);
    const int batch_size = q.size(0), seqlen_q = q.size(1), num_heads = q.size(2), d = q.size(3);
    const int page = kcache.size(1), num_heads_k = kcache.size(2);
    TORCH_CHECK(kcache.size(3) == d && d % 8 == 0 && d <= 256, "head_size must be a multiple of 8 and <= 256");
    check_heads(batch_size, num_heads, num_heads_k, d, "forward");
    auto bt = block_table.contiguous();      // (so any strides are taken)
    check_block_table(bt, batch_size);
    check_batch_int32(seqlens_k, batch_size, "seqlens_k");
    const int seqlen_k = bt.size(1) * page;
    normalize_window(is_causal, seqlen_q == 1, seqlen_k, /*clip_first=*/false, window_size_left, window_size_right);
    const c10::DeviceGuard device_guard(q.device());
    auto qc = dense(q);
    auto out = torch::empty_like(qc);
    auto lse = torch::empty({batch_size, num_heads, seqlen_q}, q.options().dtype(at::kFloat));
    fmha_page_kvcache_fwd_sink(qc.data_ptr(), kcache.data_ptr(), vcache.data_ptr(), out.data_ptr(),
                               lse.data_ptr(), bt.data_ptr(), (int)bt.stride(0), seqlens_k.data_ptr(),
                               seqlen_q, seqlen_k, batch_size, num_heads, num_heads_k, d, page,
                               softmax_scale, window_size_left, window_size_right, 0.f, nullptr, 0,
                               num_splits, 1, k_scale, v_scale, nullptr, dt == torch::kFloat16,
                               cur_stream(), sink_for_c(sink_, q, num_heads));
    raise_if_failed("fwd_kvcache_fp8");
    return {out, lse};
}

namespace {

// Device descales of the _ex ops: fp32 CUDA tensors of one element or of shape [batch, heads_k]
// (FA3's layout), brought to one stride pair for the three of them - (0, 0) when all have one
// element, else [batch, heads_k] contiguous (a one-element tensor expanded on the device: no
// host read)
struct DeviceDescales { at::Tensor q, k, v; int batch_stride, head_stride; };
DeviceDescales device_descales(const at::Tensor& qd, const at::Tensor& kd, const at::Tensor& vd,
                               const at::Tensor& like, int batch_size, int num_heads_k) {
    const at::Tensor* in[3] = {&qd, &kd, &vd};
    bool per_head = false;
    for (const at::Tensor* t : in) {
        TORCH_CHECK(t->is_cuda() && t->device() == like.device(), "descales must be CUDA tensors on q's device");
        TORCH_CHECK(t->scalar_type() == torch::kFloat32, "descales must have dtype float32");
        const bool one = t->numel() == 1;
        TORCH_CHECK(one || t->sizes() == torch::IntArrayRef({batch_size, num_heads_k}),
                    "a descale must have one element or shape (batch_size, num_heads_k)");
        per_head = per_head || !one;
    }
    at::Tensor out[3];
    for (int i = 0; i < 3; ++i)
        out[i] = !per_head ? in[i]->reshape({1})
                           : (in[i]->numel() == 1 && in[i]->dim() != 2 ? in[i]->reshape({1, 1}) : *in[i])
                                 .expand({batch_size, num_heads_k}).contiguous();
    return {out[0], out[1], out[2], per_head ? num_heads_k : 0, per_head ? 1 : 0};
}

// what the four fp8 q/k/v forwards check alike: byte-sized contiguous q, k, v of rank N on the device
template <int N>
void check_fp8_qkv(const at::Tensor& q, const at::Tensor& k, const at::Tensor& v, const char* what,
                   const char* layout) {
    TORCH_CHECK(q.element_size() == 1 && k.element_size() == 1 && v.element_size() == 1,
                what, ": q, k and v must be float8_e4m3fn (or uint8 bytes)");
    CHECK_DEVICE(q); CHECK_DEVICE(k); CHECK_DEVICE(v);
    CHECK_CONTIGUOUS(q); CHECK_CONTIGUOUS(k); CHECK_CONTIGUOUS(v);
    TORCH_CHECK(q.dim() == N && k.dim() == N && v.dim() == N, "q, k, v must be ", layout);
}

// ... and their `out`: its dtype is out_fp16's choice, not the inputs', and one the kernel cannot
// write directly is refused
at::Tensor take_fp8_out(const OptTensor& out_, const at::Tensor& q, bool out_fp16, std::vector<int64_t> shape) {
    const auto odt = out_fp16 ? torch::kFloat16 : torch::kBFloat16;
    TORCH_CHECK(!out_.has_value() || out_.value().dtype() == odt, "out has the wrong dtype");
    return take_out(out_, q.options().dtype(odt), std::move(shape), /*strided_ok=*/false, /*refuse_indirect=*/true);
}

// fp8 e4m3fn Q/K/V forward (extension): q [b, sq, h, 128], k/v [b, sk, hk, 128] as
// float8_e4m3fn (or uint8 bytes) with per-tensor descales; returns {out (out_dtype), lse}.
// `launch(out, lse, window_left, window_right)` calls the C entry (by-value or device descales)
template <typename F>
std::vector<at::Tensor>
fwd_fp8_impl(const char* op, const at::Tensor& q, const at::Tensor& k, const at::Tensor& v,
             OptTensor& out_, bool is_causal, int window_size_left, int window_size_right,
             const bool out_fp16, F&& launch) {
    check_fp8_qkv<4>(q, k, v, "fp8 forward", "[b, s, h, d]");
    const int batch_size = q.size(0), seqlen_q = q.size(1), num_heads = q.size(2), d = q.size(3);
    const int seqlen_k = k.size(1), num_heads_k = k.size(2);
    TORCH_CHECK(d == 128, "fp8 forward supports head_size 128");
    CHECK_SHAPE(k, batch_size, seqlen_k, num_heads_k, d);
    CHECK_SHAPE(v, batch_size, seqlen_k, num_heads_k, d);
    check_heads(batch_size, num_heads, num_heads_k, d, "forward");
    normalize_window(is_causal, seqlen_q == 1, seqlen_k, /*clip_first=*/false, window_size_left, window_size_right);
    const c10::DeviceGuard device_guard(q.device());
    at::Tensor out = take_fp8_out(out_, q, out_fp16, {batch_size, seqlen_q, num_heads, d});
    auto lse = torch::empty({batch_size, num_heads, seqlen_q}, q.options().dtype(at::kFloat));
    launch(out, lse, window_size_left, window_size_right);
    raise_if_failed(op);
    return {out, lse};
}

// fp8 e4m3fn forward over packed sequences (extension): q [total_q, h, 128], k/v
// [total_k, hk, 128], cu_seqlens int32 [b + 1], optional seqused_k int32 [b]; returns
// {out [total_q, h, 128] (out dtype), lse [h, total_q]}.
// `launch(out, lse, seqused pointer, window_left, window_right)` calls the C entry
template <typename F>
std::vector<at::Tensor>
varlen_fwd_fp8_impl(const char* op, const at::Tensor& q, const at::Tensor& k, const at::Tensor& v,
                    OptTensor& out_, const at::Tensor& cu_seqlens_q, const at::Tensor& cu_seqlens_k,
                    OptTensor& seqused_k, int max_seqlen_q, const int max_seqlen_k, bool is_causal,
                    int window_size_left, int window_size_right, const bool out_fp16, F&& launch) {
    check_fp8_qkv<3>(q, k, v, "fp8 varlen forward", "[total, h, d]");
    const int batch_size = check_cu_seqlens(cu_seqlens_q, cu_seqlens_k);
    TORCH_CHECK(cu_seqlens_q.device() == q.device() && cu_seqlens_k.device() == q.device(),
                "cu_seqlens must be on q's device");
    const int total_q = q.size(0), num_heads = q.size(1), d = q.size(2);
    const int total_k = k.size(0), num_heads_k = k.size(1);
    TORCH_CHECK(d == 128, "fp8 forward supports head_size 128");
    CHECK_SHAPE(k, total_k, num_heads_k, d);
    CHECK_SHAPE(v, total_k, num_heads_k, d);
    check_heads(batch_size, num_heads, num_heads_k, d, "forward");
    TORCH_CHECK(max_seqlen_q > 0 && max_seqlen_k > 0, "max_seqlen_q and max_seqlen_k must be positive");
    at::Tensor seqused = batch_int32(seqused_k, batch_size, "seqused_k");
    TORCH_CHECK(!seqused.defined() || seqused.device() == q.device(), "seqused_k must be on q's device");
    normalize_window(is_causal, max_seqlen_q == 1, max_seqlen_k, /*clip_first=*/false, window_size_left,
                     window_size_right);
    const c10::DeviceGuard device_guard(q.device());
    at::Tensor out = take_fp8_out(out_, q, out_fp16, {total_q, num_heads, d});
    auto lse = torch::empty({num_heads, total_q}, q.options().dtype(at::kFloat));
    if (total_q == 0) return {out, lse};
    launch(out, lse, ptr_or_null(seqused), window_size_left, window_size_right);
    raise_if_failed(op);
    return {out, lse};
}

}  // namespace

std::vector<at::Tensor>
mha_fwd_fp8(const at::Tensor& q, const at::Tensor& k, const at::Tensor& v, OptTensor& out_,
            const float q_scale, const float k_scale, const float v_scale, const float softmax_scale,
            bool is_causal, int window_size_left, int window_size_right, const bool out_fp16) {
    return fwd_fp8_impl("fwd_fp8", q, k, v, out_, is_causal, window_size_left, window_size_right, out_fp16,
                        [&](at::Tensor& out, at::Tensor& lse, int wl, int wr) {
        fmha_fwd_fp8(q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), lse.data_ptr(), q_scale,
                     k_scale, v_scale, q.size(1), k.size(1), q.size(0), q.size(2), k.size(2), q.size(3),
                     softmax_scale, wl, wr, out_fp16, cur_stream());
    });
}

// ... with the descales as device tensors (one element or [batch, heads_k]): no host read
std::vector<at::Tensor>
mha_fwd_fp8_ex(const at::Tensor& q, const at::Tensor& k, const at::Tensor& v, OptTensor& out_,
               const at::Tensor& q_descale, const at::Tensor& k_descale, const at::Tensor& v_descale,
               const float softmax_scale, bool is_causal, int window_size_left, int window_size_right,
               const bool out_fp16) {
    TORCH_CHECK(q.dim() == 4 && k.dim() == 4, "q, k, v must be [b, s, h, d]");
    const DeviceDescales ds = device_descales(q_descale, k_descale, v_descale, q, q.size(0), k.size(2));
    return fwd_fp8_impl("fwd_fp8_ex", q, k, v, out_, is_causal, window_size_left, window_size_right, out_fp16,
                        [&](at::Tensor& out, at::Tensor& lse, int wl, int wr) {
        fmha_fwd_fp8_ex(q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), lse.data_ptr(),
                        ds.q.data_ptr<float>(), ds.k.data_ptr<float>(), ds.v.data_ptr<float>(),
                        ds.batch_stride, ds.head_stride, q.size(1), k.size(1), q.size(0), q.size(2),
                        k.size(2), q.size(3), softmax_scale, wl, wr, out_fp16, cur_stream());
    });
}

std::vector<at::Tensor>
mha_varlen_fwd_fp8(const at::Tensor& q, const at::Tensor& k, const at::Tensor& v, OptTensor& out_,
                   const at::Tensor& cu_seqlens_q, const at::Tensor& cu_seqlens_k, OptTensor& seqused_k,
                   int max_seqlen_q, const int max_seqlen_k, const float q_scale, const float k_scale,
                   const float v_scale, const float softmax_scale, bool is_causal, int window_size_left,
                   int window_size_right, const bool out_fp16) {
    return varlen_fwd_fp8_impl("varlen_fwd_fp8", q, k, v, out_, cu_seqlens_q, cu_seqlens_k, seqused_k,
                               max_seqlen_q, max_seqlen_k, is_causal, window_size_left,
                               window_size_right, out_fp16,
                               [&](at::Tensor& out, at::Tensor& lse, void* seqused, int wl, int wr) {
        fmha_varlen_fwd_fp8(q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), lse.data_ptr(),
                            cu_seqlens_q.data_ptr(), cu_seqlens_k.data_ptr(), seqused, q_scale, k_scale,
                            v_scale, max_seqlen_q, max_seqlen_k, q.size(0), cu_seqlens_q.numel() - 1,
                            q.size(1), k.size(1), q.size(2), softmax_scale, wl, wr, out_fp16, cur_stream());
    });
}

// ... with the descales as device tensors (one element or [sequences, heads_k]): no host read
std::vector<at::Tensor>
mha_varlen_fwd_fp8_ex(const at::Tensor& q, const at::Tensor& k, const at::Tensor& v, OptTensor& out_,
                      const at::Tensor& cu_seqlens_q, const at::Tensor& cu_seqlens_k, OptTensor& seqused_k,
                      int max_seqlen_q, const int max_seqlen_k, const at::Tensor& q_descale,
                      const at::Tensor& k_descale, const at::Tensor& v_descale, const float softmax_scale,
                      bool is_causal, int window_size_left, int window_size_right, const bool out_fp16) {
    TORCH_CHECK(q.dim() == 3 && k.dim() == 3, "q, k, v must be [total, h, d]");
    const DeviceDescales ds = device_descales(q_descale, k_descale, v_descale, q,
                                              (int)cu_seqlens_q.numel() - 1, k.size(1));
    return varlen_fwd_fp8_impl("varlen_fwd_fp8_ex", q, k, v, out_, cu_seqlens_q, cu_seqlens_k, seqused_k,
                               max_seqlen_q, max_seqlen_k, is_causal, window_size_left,
                               window_size_right, out_fp16,
                               [&](at::Tensor& out, at::Tensor& lse, void* seqused, int wl, int wr) {
        fmha_varlen_fwd_fp8_ex(q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), lse.data_ptr(),
                               cu_seqlens_q.data_ptr(), cu_seqlens_k.data_ptr(), seqused,
                               ds.q.data_ptr<float>(), ds.k.data_ptr<float>(), ds.v.data_ptr<float>(),
                               ds.batch_stride, ds.head_stride, max_seqlen_q, max_seqlen_k, q.size(0),
                               cu_seqlens_q.numel() - 1, q.size(1), k.size(1), q.size(2), softmax_scale,
                               wl, wr, out_fp16, cur_stream());
    });
}

// bf16 / fp16 -> fp8 e4m3fn with its descale(s) (fmha_quantize_fp8): x [b, s, h, d] (any strides
// with a contiguous last dimension) or, with cu_seqlens, packed [total, h, d] (max_seqlen <= 0:
// total bounds a sequence's rows, so no length is read on the host); granularity 0 one scale,
// 1 one per (batch or sequence, group of `group` heads).  Returns {x8 (float8_e4m3fn,
// contiguous), descale fp32 [1] or [b, h / group]}.
std::vector<at::Tensor>
mha_quantize_fp8(const at::Tensor& x, int granularity, int group, OptTensor& cu_seqlens_, int max_seqlen) {
    auto dt = x.dtype();
    TORCH_CHECK(dt == torch::kFloat16 || dt == torch::kBFloat16, "quantize_fp8: x must be fp16 or bf16");
    CHECK_DEVICE(x);
    TORCH_CHECK(granularity == 0 || granularity == 1, "granularity must be 0 (tensor) or 1 (head)");
    const bool packed = cu_seqlens_.has_value();
    TORCH_CHECK(x.dim() == (packed ? 3 : 4), "x must be [b, s, h, d], or [total, h, d] with cu_seqlens");
    at::Tensor xs = x.stride(-1) == 1 && aligned16(x) ? x : dense(x);
    const c10::DeviceGuard device_guard(x.device());
    at::Tensor cu;
    int batch_size, seqlen, num_heads, d;
    int64_t st[3];
    if (packed) {
        cu = cu_seqlens_.value();
        batch_size = check_cu_seqlens(cu, "cu_seqlens");
        TORCH_CHECK(cu.device() == x.device(), "cu_seqlens must be on x's device");
        seqlen = max_seqlen > 0 ? max_seqlen : (int)xs.size(0);
        num_heads = xs.size(1); d = xs.size(2);
        st[0] = 0; st[1] = xs.stride(0); st[2] = xs.stride(1);
    } else {
        batch_size = xs.size(0); seqlen = xs.size(1); num_heads = xs.size(2); d = xs.size(3);
        st[0] = xs.stride(0); st[1] = xs.stride(1); st[2] = xs.stride(2);
    }
    TORCH_CHECK(group > 0 && num_heads % group == 0, "group must divide the number of heads");
    auto x8 = torch::empty(xs.sizes(), x.options().dtype(at::kFloat8_e4m3fn));
    auto descale = granularity ? torch::empty({batch_size, num_heads / group}, x.options().dtype(at::kFloat))
                               : torch::empty({1}, x.options().dtype(at::kFloat));
    if (xs.numel() == 0) { descale.fill_(1.f); return {x8, descale}; }
    fmha_quantize_fp8(xs.data_ptr(), x8.data_ptr(), descale.data_ptr<float>(), ptr_or_null(cu), batch_size,
                      seqlen, num_heads, group, d, st, granularity, dt == torch::kFloat16, cur_stream());
    raise_if_failed("quantize_fp8");
    return {x8, descale};
}

// Append new K/V rows (+ rotary on k and q) into an fp8 e4m3fn paged cache
// (fmha_kvcache_append_fp8): the write step of fwd_kvcache for an fp8 cache.  Returns
// {seqlens_out, q_out (rotary; else q itself)}.
std::vector<at::Tensor>
mha_kvcache_append_fp8(const at::Tensor& q, at::Tensor& kcache, at::Tensor& vcache, const at::Tensor& kn,
                       const at::Tensor& vn, const at::Tensor& seqlens_k, const at::Tensor& block_table,
                       OptTensor& rotary_cos_, OptTensor& rotary_sin_, const float k_scale,
                       const float v_scale, bool is_rotary_interleaved, bool q_rotary_per_token) {
    auto dt = q.dtype();
    TORCH_CHECK(dt == torch::kFloat16 || dt == torch::kBFloat16, "q must be fp16 or bf16");
    TORCH_CHECK(kn.dtype() == dt && vn.dtype() == dt, "new key / value must have the same dtype as query");
    TORCH_CHECK(kcache.element_size() == 1 && vcache.element_size() == 1, "fp8 K/V cache expected");
    CHECK_DEVICE(q); CHECK_DEVICE(kcache); CHECK_DEVICE(vcache); CHECK_DEVICE(kn); CHECK_DEVICE(vn);
    CHECK_CONTIGUOUS(kcache); CHECK_CONTIGUOUS(vcache);
    TORCH_CHECK(q.dim() == 4 && kn.dim() == 4 && kcache.dim() == 4 && block_table.dim() == 2,
                "q, k, v, caches must be 4-D and block_table 2-D");
    const int batch_size = q.size(0), seqlen_q = q.size(1), num_heads = q.size(2), d = q.size(3);
    const int page = kcache.size(1), num_heads_k = kcache.size(2), seqlen_new = kn.size(1);
    TORCH_CHECK(kcache.size(3) == d && d % 8 == 0 && d <= 256, "head_size must be a multiple of 8 and <= 256");
    check_heads(batch_size, num_heads, num_heads_k, d, "forward");
    TORCH_CHECK(vcache.sizes() == kcache.sizes(), "k_cache and v_cache must have the same shape");
    CHECK_SHAPE(kn, batch_size, seqlen_new, num_heads_k, d);
    CHECK_SHAPE(vn, batch_size, seqlen_new, num_heads_k, d);
    auto bt = block_table.contiguous();      // (so any strides are taken)
    check_block_table(bt, batch_size);
    check_batch_int32(seqlens_k, batch_size, "seqlens_k");
    TORCH_CHECK(k_scale > 0.f && v_scale > 0.f, "fp8 cache descales must be positive");
    const c10::DeviceGuard device_guard(q.device());
    auto qc = dense(q);
    auto knc = dense(kn), vnc = dense(vn);
    TORCH_CHECK(!rotary_cos_.has_value() || rotary_cos_.value().dim() == 2,
                "rotary_cos must be [seqlen_ro, rotary_dim / 2]");
    const Rotary rotary = check_rotary(rotary_cos_, rotary_sin_, q, d, (int64_t)bt.size(1) * page);
    at::Tensor q_rot = rotary.cos.defined() ? torch::empty_like(qc) : at::Tensor();
    auto seqlens_new = torch::empty_like(seqlens_k);
    fmha_kvcache_append_fp8(qc.data_ptr(), ptr_or_null(q_rot), kcache.data_ptr(), vcache.data_ptr(),
                            knc.data_ptr(), vnc.data_ptr(), seqlen_new, bt.data_ptr(), (int)bt.stride(0), page,
                            seqlens_k.data_ptr(), seqlens_new.data_ptr(), ptr_or_null(rotary.cos),
                            ptr_or_null(rotary.sin), rotary.dim, is_rotary_interleaved, q_rotary_per_token,
                            batch_size, seqlen_q, num_heads, num_heads_k, d, dt == torch::kFloat16,
                            cur_stream(), k_scale, v_scale);
    raise_if_failed("kvcache_append_fp8");
    return {seqlens_new, q_rot.defined() ? q_rot : qc};
}

namespace {

// ---- `mla_decode`: q [batch, seqlen_q, heads, 576], fp16 or bf16, by its own strides ...
void check_mla_q(const at::Tensor& q) {
    TORCH_CHECK(q.dtype() == torch::kFloat16 || q.dtype() == torch::kBFloat16, "q must be fp16 or bf16");
    CHECK_DEVICE(q);
    TORCH_CHECK(q.dim() == 4, "q must be ", kDense);
    TORCH_CHECK(q.size(3) == 576, "mla_decode takes head_size 576 (512 latent + 64 rotary features), got ", q.size(3));
    TORCH_CHECK(q.size(1) >= 1 && q.size(2) >= 1, "q must have at least one row and one head");
    TORCH_CHECK(q.stride(-1) == 1, "q must have contiguous last dimension");
    TORCH_CHECK(aligned16(q), "q must be 16-byte aligned with strides that are multiples of 16 bytes");
}

// ... the latent cache [num_blocks, page, 1, 576] of q's dtype, contiguous (fp8: bytes
// [num_blocks, page, 1, 656], uint8 or float8_e4m3fn) ...
bool is_byte_cache(const at::Tensor& kv_cache) {
    return kv_cache.dtype() == torch::kUInt8 || kv_cache.dtype() == at::kFloat8_e4m3fn;
}
void check_mla_cache(const at::Tensor& kv_cache, const at::Tensor& q, bool fp8 = false) {
    TORCH_CHECK(!fp8 || is_byte_cache(kv_cache), "kv_cache must be uint8 or float8_e4m3fn (rows of 656 bytes)");
    TORCH_CHECK(fp8 || kv_cache.dtype() == q.dtype(), "kv_cache must have the dtype of q");
    TORCH_CHECK(kv_cache.is_cuda() && kv_cache.device() == q.device(), "kv_cache must be on q's device");
    TORCH_CHECK(kv_cache.dim() == 4 && kv_cache.size(2) == 1 && kv_cache.size(3) == (fp8 ? 656 : 576),
                "kv_cache must be (num_blocks, page_block_size, 1, ", fp8 ? 656 : 576, ")");
    CHECK_CONTIGUOUS(kv_cache);
    TORCH_CHECK(kv_cache.size(1) % 16 == 0, "page_block_size must be a multiple of 16");
    TORCH_CHECK(aligned16(kv_cache), "kv_cache must be 16-byte aligned");
}

// ... and an output: the caller's (written in place by its own strides) or a new contiguous one
at::Tensor take_mla_out(const OptTensor& out_, const at::Tensor& q, int head_size_v) {
    const std::vector<int64_t> shape = {q.size(0), q.size(1), q.size(2), head_size_v};
    if (!out_.has_value()) return torch::empty(shape, q.options());
    const at::Tensor& out = out_.value();
    TORCH_CHECK(out.dtype() == q.dtype(), "Output must have the same dtype as inputs");
    TORCH_CHECK(out.is_cuda() && out.device() == q.device(), "out must be on q's device");
    TORCH_CHECK(out.sizes() == at::IntArrayRef(shape), "out must have shape ", at::IntArrayRef(shape));
    TORCH_CHECK(out.stride(-1) == 1, "Output tensor must have contiguous last dimension");
    TORCH_CHECK(aligned16(out), "out must be 16-byte aligned with strides that are multiples of 16 bytes");
    return out;
}

// ... and, for the sparse decode, the indexer's choice: int32 [batch, seqlen_q, topk] of q's batch
// and seqlen_q, by its own batch and row strides
void check_mla_indices(const at::Tensor& indices, const at::Tensor& q) {
    TORCH_CHECK(indices.dtype() == torch::kInt32, "indices must have dtype int32");
    TORCH_CHECK(indices.is_cuda() && indices.device() == q.device(), "indices must be on q's device");
    TORCH_CHECK(indices.dim() == 3 && indices.size(0) == q.size(0) && indices.size(1) == q.size(1),
                "indices must be (batch_size, seqlen_q, topk) with q's batch_size and seqlen_q");
    TORCH_CHECK(indices.size(2) >= 1, "indices must hold at least one entry per query position (topk >= 1)");
    TORCH_CHECK(indices.stride(2) == 1 || indices.size(2) == 1, "indices must have contiguous last dimension");
    TORCH_CHECK(indices.stride(0) >= 0 && indices.stride(1) >= 0, "indices must have non-negative strides");
}

}  // namespace

// MLA decode over a paged latent cache (fmha_mla_decode; fp8: fmha_mla_decode_fp8 over rows of 656
// bytes): q and out go by their own strides, nothing is copied.  Returns {out [batch, seqlen_q,
// heads, 512], softmax_lse [batch, heads, seqlen_q]}.
template <bool kFp8>
std::vector<at::Tensor>
mha_mla_decode(const at::Tensor& q, const at::Tensor& kv_cache, const at::Tensor& block_table,
               const at::Tensor& cache_seqlens, const int head_dim_v, const float softmax_scale,
               const bool is_causal, const int num_splits, const OptTensor& out_) {
    check_mla_q(q);
    check_mla_cache(kv_cache, q, kFp8);
    TORCH_CHECK(head_dim_v == 512, "mla_decode takes head_dim_v 512, got ", head_dim_v);
    const int batch = q.size(0), seqlen_q = q.size(1), heads = q.size(2);
    TORCH_CHECK(block_table.dim() == 2, "block_table must be (batch_size, max_num_blocks_per_seq)");
    check_block_table(block_table, batch);
    check_batch_int32(cache_seqlens, batch, "cache_seqlens");
    TORCH_CHECK(block_table.device() == q.device() && cache_seqlens.device() == q.device(),
                "block_table and cache_seqlens must be on q's device");
    TORCH_CHECK(num_splits <= 128, "num_splits must be at most 128");
    at::Tensor out = take_mla_out(out_, q, head_dim_v);
    at::Tensor lse = torch::empty({batch, heads, seqlen_q}, q.options().dtype(torch::kFloat32));
    if (batch == 0) return {out, lse};
    const c10::DeviceGuard device_guard(q.device());
    const int page = kv_cache.size(1);
    const int64_t st[6] = {q.stride(0), q.stride(1), q.stride(2), out.stride(0), out.stride(1), out.stride(2)};
    (kFp8 ? fmha_mla_decode_fp8 : fmha_mla_decode)(
        q.data_ptr(), kv_cache.data_ptr(), out.data_ptr(), lse.data_ptr(), block_table.data_ptr(),
        (int)block_table.stride(0), cache_seqlens.data_ptr(), seqlen_q,
        (int)std::min<int64_t>(block_table.size(1) * (int64_t)page, 0x7fffffff), batch, heads, 576,
        head_dim_v, page, st, softmax_scale, -1, is_causal ? 0 : -1, num_splits,
        q.dtype() == torch::kFloat16, cur_stream());
    raise_if_failed(kFp8 ? "mla_decode_fp8" : "mla_decode");
    return {out, lse};
}

// MLA decode over index-selected tokens (fmha_mla_decode_sparse; fp8: fmha_mla_decode_sparse_fp8):
// the keys of query (b, pos) are the cache rows at the valid entries of indices[b, pos, :], physical
// slots block * page + row.  The kernel validates the entries; nothing is copied or synchronised.
template <bool kFp8>
std::vector<at::Tensor>
mha_mla_decode_sparse(const at::Tensor& q, const at::Tensor& kv_cache, const at::Tensor& indices,
                      const int head_dim_v, const float softmax_scale, const int num_splits,
                      const OptTensor& out_) {
    check_mla_q(q);
    check_mla_cache(kv_cache, q, kFp8);
    check_mla_indices(indices, q);
    TORCH_CHECK(head_dim_v == 512, "mla_decode_sparse takes head_dim_v 512, got ", head_dim_v);
    TORCH_CHECK(kv_cache.size(0) >= 1 && kv_cache.size(1) >= 16, "kv_cache must hold at least one page");
    TORCH_CHECK(kv_cache.size(0) <= 0x7fffffff && indices.size(2) <= 0x7fffffff, "kv_cache or indices too large");
    TORCH_CHECK(num_splits <= 128, "num_splits must be at most 128");
    const int batch = q.size(0), seqlen_q = q.size(1), heads = q.size(2);
    at::Tensor out = take_mla_out(out_, q, head_dim_v);
    at::Tensor lse = torch::empty({batch, heads, seqlen_q}, q.options().dtype(torch::kFloat32));
    if (batch == 0) return {out, lse};
    const c10::DeviceGuard device_guard(q.device());
    const int64_t st[6] = {q.stride(0), q.stride(1), q.stride(2), out.stride(0), out.stride(1), out.stride(2)};
    (kFp8 ? fmha_mla_decode_sparse_fp8 : fmha_mla_decode_sparse)(
        q.data_ptr(), kv_cache.data_ptr(), out.data_ptr(), lse.data_ptr(), indices.data_ptr(),
        indices.stride(0), indices.stride(1), (int)indices.size(2), seqlen_q, batch, heads, 576, head_dim_v,
        (int)kv_cache.size(0), (int)kv_cache.size(1), st, softmax_scale, num_splits,
        q.dtype() == torch::kFloat16, cur_stream());
    raise_if_failed(kFp8 ? "mla_decode_sparse_fp8" : "mla_decode_sparse");
    return {out, lse};
}

// Append tokens to the fp8 latent cache (fmha_mla_cache_append_fp8): latent [tokens, 512] and k_pe
// [tokens, 64] by their own row strides (views of one 576-wide tensor are fine), slot_mapping int64.
void mha_mla_cache_append_fp8(const at::Tensor& latent, const at::Tensor& k_pe, at::Tensor& kv_cache,
                              const at::Tensor& slot_mapping) {
    auto dt = latent.dtype();
    TORCH_CHECK(dt == torch::kFloat16 || dt == torch::kBFloat16, "latent must be fp16 or bf16");
    TORCH_CHECK(k_pe.dtype() == dt, "k_pe must have the dtype of latent");
    CHECK_DEVICE(latent); CHECK_DEVICE(k_pe); CHECK_DEVICE(kv_cache); CHECK_DEVICE(slot_mapping);
    TORCH_CHECK(k_pe.device() == latent.device() && kv_cache.device() == latent.device() &&
                    slot_mapping.device() == latent.device(), "all tensors must be on one device");
    TORCH_CHECK(latent.dim() == 2 && latent.size(1) == 512, "latent must be (num_tokens, 512)");
    TORCH_CHECK(k_pe.dim() == 2 && k_pe.size(1) == 64 && k_pe.size(0) == latent.size(0),
                "k_pe must be (num_tokens, 64)");
    TORCH_CHECK(latent.stride(1) == 1 && k_pe.stride(1) == 1, "latent and k_pe must have contiguous last dimension");
    TORCH_CHECK(aligned16(latent) && aligned16(k_pe),
                "latent and k_pe must be 16-byte aligned with row strides that are multiples of 16 bytes");
    TORCH_CHECK(is_byte_cache(kv_cache), "kv_cache must be uint8 or float8_e4m3fn (rows of 656 bytes)");
    TORCH_CHECK(kv_cache.dim() == 4 && kv_cache.size(2) == 1 && kv_cache.size(3) == 656,
                "kv_cache must be (num_blocks, page_block_size, 1, 656)");
    CHECK_CONTIGUOUS(kv_cache);
    TORCH_CHECK(kv_cache.size(1) % 16 == 0, "page_block_size must be a multiple of 16");
    TORCH_CHECK(aligned16(kv_cache), "kv_cache must be 16-byte aligned");
    TORCH_CHECK(slot_mapping.dtype() == torch::kInt64 && slot_mapping.dim() == 1 &&
                    slot_mapping.size(0) == latent.size(0) && slot_mapping.is_contiguous(),
                "slot_mapping must be a contiguous int64 (num_tokens)");
    if (latent.size(0) == 0) return;
    const c10::DeviceGuard device_guard(latent.device());
    fmha_mla_cache_append_fp8(latent.data_ptr(), latent.stride(0), k_pe.data_ptr(), k_pe.stride(0),
                              kv_cache.data_ptr(), slot_mapping.data_ptr(), (int)latent.size(0),
                              (int)kv_cache.size(0), (int)kv_cache.size(1), dt == torch::kFloat16, cur_stream());
    raise_if_failed("mla_cache_append_fp8");
}

namespace {

// ---- `fwd_mla` / `varlen_fwd_mla`: q and k with 192 features a head, v with 128, each by its own
// strides.  Nothing is padded or copied: a tensor the kernel cannot read as it stands is refused.
void check_mla_prefill_tensor(const at::Tensor& t, const at::Tensor& q, const char* name) {
    TORCH_CHECK(t.dtype() == q.dtype(), name, " must have the dtype of q");
    TORCH_CHECK(t.is_cuda() && t.device() == q.device(), name, " must be on q's device");
    TORCH_CHECK(t.stride(-1) == 1, name, " must have contiguous last dimension");
    TORCH_CHECK(aligned16(t), name, " must be 16-byte aligned with strides that are multiples of 16 bytes");
}
// the pair of head sizes, the head counts and the four tensors; `rank` 4 (dense) or 3 (packed)
void check_mla_prefill(const at::Tensor& q, const at::Tensor& k, const at::Tensor& v, int rank) {
    TORCH_CHECK(q.dtype() == torch::kFloat16 || q.dtype() == torch::kBFloat16, "q must be fp16 or bf16");
    CHECK_DEVICE(q);
    const char* layout = rank == 4 ? kDense : kPacked;
    TORCH_CHECK(q.dim() == rank, "q must be ", layout);
    TORCH_CHECK(k.dim() == rank, "k must be ", layout);
    TORCH_CHECK(v.dim() == rank, "v must be ", layout);
    TORCH_CHECK(q.size(-1) == 192 && k.size(-1) == 192 && v.size(-1) == 128,
                "MLA prefill supports (head_size_qk, head_size_v) = (192, 128) only (got q ", q.size(-1),
                ", k ", k.size(-1), ", v ", v.size(-1), ")");
    check_mla_prefill_tensor(q, q, "q");
    check_mla_prefill_tensor(k, q, "k");
    check_mla_prefill_tensor(v, q, "v");
    TORCH_CHECK(k.size(-2) == v.size(-2), "k and v must have the same number of heads");
    TORCH_CHECK(k.size(-3) == v.size(-3), "k and v must have the same number of rows");
    TORCH_CHECK(q.size(-2) >= 1 && k.size(-2) >= 1 && q.size(-2) % k.size(-2) == 0,
                "Number of heads in key/value must divide number of heads in query");
}
// the caller's output (written in place by its own strides) or a new contiguous one
at::Tensor take_mla_prefill_out(const OptTensor& out_, const at::Tensor& q) {
    std::vector<int64_t> shape = q.sizes().vec();
    shape.back() = 128;
    if (!out_.has_value()) return torch::empty(shape, q.options());
    const at::Tensor& out = out_.value();
    TORCH_CHECK(out.sizes() == at::IntArrayRef(shape), "out must have shape ", at::IntArrayRef(shape));
    check_mla_prefill_tensor(out, q, "out");
    return out;
}

}  // namespace

// MLA prefill, dense (fmha_fwd_mla).  Returns {out [batch, seqlen_q, heads, 128], softmax_lse
// [batch, heads, seqlen_q]}.
std::vector<at::Tensor>
mha_fwd_mla(const at::Tensor& q, const at::Tensor& k, const at::Tensor& v, const OptTensor& out_,
            const float softmax_scale, const bool is_causal, int window_size_left, int window_size_right) {
    check_mla_prefill(q, k, v, 4);
    const int batch = q.size(0), seqlen_q = q.size(1), heads = q.size(2);
    const int seqlen_k = k.size(1), heads_k = k.size(2);
    TORCH_CHECK(batch > 0, "batch size must be positive");
    TORCH_CHECK(k.size(0) == batch && v.size(0) == batch, "k and v must have q's batch size");
    TORCH_CHECK(seqlen_q > 0 && seqlen_k > 0, "seqlen_q and seqlen_k must be positive");
    normalize_window(is_causal, false, seqlen_k, false, window_size_left, window_size_right);
    at::Tensor out = take_mla_prefill_out(out_, q);
    at::Tensor lse = torch::empty({batch, heads, seqlen_q}, q.options().dtype(torch::kFloat32));
    const c10::DeviceGuard device_guard(q.device());
    const int64_t st[12] = {q.stride(0), q.stride(1), q.stride(2), k.stride(0), k.stride(1), k.stride(2),
                            v.stride(0), v.stride(1), v.stride(2), out.stride(0), out.stride(1), out.stride(2)};
    fmha_fwd_mla(q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), lse.data_ptr(), seqlen_q, seqlen_k,
                 batch, heads, heads_k, 192, 128, st, softmax_scale, window_size_left, window_size_right,
                 q.dtype() == torch::kFloat16, cur_stream());
    raise_if_failed("fwd_mla");
    return {out, lse};
}

// MLA prefill, packed (fmha_varlen_fwd_mla).  Returns {out [total_q, heads, 128], softmax_lse
// [heads, total_q]}.
std::vector<at::Tensor>
mha_varlen_fwd_mla(const at::Tensor& q, const at::Tensor& k, const at::Tensor& v, const OptTensor& out_,
                   const at::Tensor& cu_seqlens_q, const at::Tensor& cu_seqlens_k, const OptTensor& seqused_k_,
                   const int max_seqlen_q, const int max_seqlen_k, const float softmax_scale,
                   const bool is_causal, int window_size_left, int window_size_right) {
    check_mla_prefill(q, k, v, 3);
    const int batch = check_cu_seqlens(cu_seqlens_q, cu_seqlens_k);
    const at::Tensor seqused_k = batch_int32(seqused_k_, batch, "seqused_k");
    TORCH_CHECK(cu_seqlens_q.device() == q.device() && cu_seqlens_k.device() == q.device() &&
                    (!seqused_k.defined() || seqused_k.device() == q.device()),
                "cu_seqlens_q, cu_seqlens_k and seqused_k must be on q's device");
    const int total_q = q.size(0), heads = q.size(1), heads_k = k.size(1);
    TORCH_CHECK(total_q > 0 && max_seqlen_q > 0, "total_q and max_seqlen_q must be positive");
    TORCH_CHECK(max_seqlen_k > 0, "max_seqlen_k must be positive: nothing to attend to");
    normalize_window(is_causal, false, max_seqlen_k, false, window_size_left, window_size_right);
    at::Tensor out = take_mla_prefill_out(out_, q);
    at::Tensor lse = torch::empty({heads, total_q}, q.options().dtype(torch::kFloat32));
    const c10::DeviceGuard device_guard(q.device());
    const int64_t st[8] = {q.stride(0), q.stride(1), k.stride(0), k.stride(1),
                           v.stride(0), v.stride(1), out.stride(0), out.stride(1)};
    fmha_varlen_fwd_mla(q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), lse.data_ptr(),
                        cu_seqlens_q.data_ptr(), cu_seqlens_k.data_ptr(), ptr_or_null(seqused_k), max_seqlen_q,
                        max_seqlen_k, total_q, batch, heads, heads_k, 192, 128, st, softmax_scale,
                        window_size_left, window_size_right, q.dtype() == torch::kFloat16, cur_stream());
    raise_if_failed("varlen_fwd_mla");
    return {out, lse};
}

namespace {

// ---- `bwd_mla` / `varlen_bwd_mla`: the gradient of the two above.  out and dout are like the
// forward's out, dq / dk / dv like q / k / v (the caller's, written in place by their own strides,
// or new contiguous ones); nothing is padded or copied.
void check_mla_bwd_like(const at::Tensor& t, const at::Tensor& q, std::vector<int64_t> shape, int width,
                        const char* name) {
    shape.back() = width;
    TORCH_CHECK(t.sizes() == at::IntArrayRef(shape), name, " must have shape ", at::IntArrayRef(shape));
    check_mla_prefill_tensor(t, q, name);
}
at::Tensor take_mla_grad(const OptTensor& g_, const at::Tensor& like, const at::Tensor& q, const char* name) {
    if (!g_.has_value()) return torch::empty(like.sizes(), like.options());
    check_mla_bwd_like(g_.value(), q, like.sizes().vec(), (int)like.size(-1), name);
    return g_.value();
}
void check_mla_lse(const at::Tensor& lse, const at::Tensor& q, at::IntArrayRef shape) {
    TORCH_CHECK(lse.dtype() == torch::kFloat32, "softmax_lse must be fp32");
    TORCH_CHECK(lse.is_cuda() && lse.device() == q.device(), "softmax_lse must be on q's device");
    TORCH_CHECK(lse.sizes() == shape, "softmax_lse must have shape ", shape);
    TORCH_CHECK(lse.is_contiguous(), "softmax_lse must be contiguous");
}
// the first `per` strides ({batch, row, head} dense, {row, head} packed) of the eight tensors, in
// the C entries' order
std::vector<int64_t> mla_bwd_strides(const at::Tensor* const (&t)[8], int per) {
    std::vector<int64_t> st;
    for (const at::Tensor* x : t)
        for (int i = 0; i < per; ++i) st.push_back(x->stride(i));
    return st;
}

}  // namespace

// MLA prefill backward, dense (fmha_bwd_mla).  Returns {dq, dk, dv, softmax_d [batch, heads, seqlen_q]}.
std::vector<at::Tensor>
mha_bwd_mla(const at::Tensor& dout, const at::Tensor& q, const at::Tensor& k, const at::Tensor& v,
            const at::Tensor& out, const at::Tensor& softmax_lse, const OptTensor& dq_, const OptTensor& dk_,
            const OptTensor& dv_, const float softmax_scale, const bool is_causal, int window_size_left,
            int window_size_right) {
    check_mla_prefill(q, k, v, 4);
    const int batch = q.size(0), seqlen_q = q.size(1), heads = q.size(2);
    const int seqlen_k = k.size(1), heads_k = k.size(2);
    TORCH_CHECK(batch > 0, "batch size must be positive");
    TORCH_CHECK(k.size(0) == batch && v.size(0) == batch, "k and v must have q's batch size");
    TORCH_CHECK(seqlen_q > 0 && seqlen_k > 0, "seqlen_q and seqlen_k must be positive");
    check_mla_bwd_like(out, q, q.sizes().vec(), 128, "out");
    check_mla_bwd_like(dout, q, q.sizes().vec(), 128, "dout");
    check_mla_lse(softmax_lse, q, {batch, heads, seqlen_q});
    normalize_window(is_causal, false, seqlen_k, false, window_size_left, window_size_right);
    at::Tensor dq = take_mla_grad(dq_, q, q, "dq"), dk = take_mla_grad(dk_, k, q, "dk"), dv = take_mla_grad(dv_, v, q, "dv");
    at::Tensor softmax_d = torch::empty({batch, heads, seqlen_q}, q.options().dtype(torch::kFloat32));
    const c10::DeviceGuard device_guard(q.device());
    const at::Tensor* const ts[8] = {&q, &k, &v, &out, &dout, &dq, &dk, &dv};
    const std::vector<int64_t> st = mla_bwd_strides(ts, 3);
    fmha_bwd_mla(dout.data_ptr(), q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), softmax_lse.data_ptr(),
                 dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), softmax_d.data_ptr(), seqlen_q, seqlen_k, batch,
                 heads, heads_k, 192, 128, st.data(), softmax_scale, window_size_left, window_size_right,
                 q.dtype() == torch::kFloat16, cur_stream());
    raise_if_failed("bwd_mla");
    return {dq, dk, dv, softmax_d};
}

// MLA prefill backward, packed (fmha_varlen_bwd_mla).  Returns {dq, dk, dv, softmax_d [heads, total_q]}.
std::vector<at::Tensor>
mha_varlen_bwd_mla(const at::Tensor& dout, const at::Tensor& q, const at::Tensor& k, const at::Tensor& v,
                   const at::Tensor& out, const at::Tensor& softmax_lse, const OptTensor& dq_,
                   const OptTensor& dk_, const OptTensor& dv_, const at::Tensor& cu_seqlens_q,
                   const at::Tensor& cu_seqlens_k, const int max_seqlen_q, const int max_seqlen_k,
                   const float softmax_scale, const bool is_causal, int window_size_left,
                   int window_size_right) {
    check_mla_prefill(q, k, v, 3);
    const int batch = check_cu_seqlens(cu_seqlens_q, cu_seqlens_k);
    TORCH_CHECK(cu_seqlens_q.device() == q.device() && cu_seqlens_k.device() == q.device(),
                "cu_seqlens_q and cu_seqlens_k must be on q's device");
    const int total_q = q.size(0), total_k = k.size(0), heads = q.size(1), heads_k = k.size(1);
    TORCH_CHECK(total_q > 0 && max_seqlen_q > 0, "total_q and max_seqlen_q must be positive");
    TORCH_CHECK(total_k > 0 && max_seqlen_k > 0, "total_k and max_seqlen_k must be positive: nothing to attend to");
    check_mla_bwd_like(out, q, q.sizes().vec(), 128, "out");
    check_mla_bwd_like(dout, q, q.sizes().vec(), 128, "dout");
    check_mla_lse(softmax_lse, q, {heads, total_q});
    normalize_window(is_causal, false, max_seqlen_k, false, window_size_left, window_size_right);
    at::Tensor dq = take_mla_grad(dq_, q, q, "dq"), dk = take_mla_grad(dk_, k, q, "dk"), dv = take_mla_grad(dv_, v, q, "dv");
    at::Tensor softmax_d = torch::empty({heads, total_q}, q.options().dtype(torch::kFloat32));
    const c10::DeviceGuard device_guard(q.device());
    const at::Tensor* const ts[8] = {&q, &k, &v, &out, &dout, &dq, &dk, &dv};
    const std::vector<int64_t> st = mla_bwd_strides(ts, 2);
    fmha_varlen_bwd_mla(dout.data_ptr(), q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(),
                        softmax_lse.data_ptr(), dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), softmax_d.data_ptr(),
                        cu_seqlens_q.data_ptr(), cu_seqlens_k.data_ptr(), max_seqlen_q, max_seqlen_k, total_q,
                        total_k, batch, heads, heads_k, 192, 128, st.data(), softmax_scale, window_size_left,
                        window_size_right, q.dtype() == torch::kFloat16, cur_stream());
    raise_if_failed("varlen_bwd_mla");
    return {dq, dk, dv, softmax_d};
}

PYBIND11_MODULE(paged_attn, m) {
    m.doc() = "FlashAttention for MI355X (gfx950): hand-written HIP kernels behind the paged_attn C ABI";
    m.def("fwd", without_sink(&mha_fwd), "Forward pass");
    m.def("varlen_fwd", without_sink(&mha_varlen_fwd), "Forward pass (variable length)");
    // the reference's positional signature (export.cpp:1757) plus an optional trailing
    // cache_leftpad
    m.def("fwd_kvcache", without_sink(&mha_fwd_kvcache), "Forward pass, with KV-cache", py::arg("q"),
          py::arg("kcache"), py::arg("vcache"), py::arg("k"), py::arg("v"), py::arg("seqlens_k"),
          py::arg("rotary_cos"), py::arg("rotary_sin"), py::arg("cache_batch_idx"),
          py::arg("block_table"), py::arg("alibi_slopes"), py::arg("out"),
          py::arg("softmax_scale"), py::arg("is_causal"), py::arg("window_size_left"),
          py::arg("window_size_right"), py::arg("softcap"), py::arg("is_rotary_interleaved"),
          py::arg("num_splits"), py::arg("cache_leftpad") = py::none());
    m.def("fwd_sink", with_sink(&mha_fwd), "Forward pass with a per-head attention sink");
    m.def("varlen_fwd_sink", with_sink(&mha_varlen_fwd), "Forward pass (variable length) with an attention sink");
    m.def("fwd_kvcache_sink", with_sink(&mha_fwd_kvcache), "Forward pass with KV-cache and an attention sink");
    m.def("fwd_kvcache_fp8_sink", with_sink(&mha_fwd_kvcache_fp8), "Paged decode over an fp8 K/V cache with an attention sink");
    m.def("sink_bwd", &mha_sink_bwd, "Gradient of the attention sink from softmax_lse and softmax_d");
    m.def("bwd", &mha_bwd, "Backward pass");
    m.def("varlen_bwd", &mha_varlen_bwd, "Backward pass (variable length)");
    m.def("fwd_kvcache_fp8", without_sink(&mha_fwd_kvcache_fp8), "Paged decode over an fp8 e4m3fn K/V cache");
    m.def("fwd_fp8", &mha_fwd_fp8, "Forward pass over fp8 e4m3fn q/k/v (fp8 MFMA)");
    m.def("varlen_fwd_fp8", &mha_varlen_fwd_fp8, "Forward pass over packed fp8 e4m3fn q/k/v (variable length)");
    m.def("quantize_fp8", &mha_quantize_fp8, "bf16 / fp16 -> fp8 e4m3fn with its descale(s)", py::arg("x"),
          py::arg("granularity"), py::arg("group"), py::arg("cu_seqlens") = py::none(),
          py::arg("max_seqlen") = 0);
    m.def("fwd_fp8_ex", &mha_fwd_fp8_ex, "fp8 forward with device descales (one element or [b, hk])");
    m.def("varlen_fwd_fp8_ex", &mha_varlen_fwd_fp8_ex, "Packed fp8 forward with device descales");
    m.def("kvcache_append_fp8", &mha_kvcache_append_fp8, "Append new K/V (+ rotary) into an fp8 e4m3fn paged cache");
    // `merge_states` is not an attention op over q / k / v and stays out of the module's listed op
    // table (dir(): the ops tests/test_ops_validation_gpu.py pins one-defect rows for, each with the
    // reference's argument list).  It is bound as `_merge_states` and resolved by name through the
    // module's __getattr__ (PEP 562): `paged_attn.merge_states(...)` is that function.  Its own
    // one-defect rows are tests/test_merge_ops_validation_gpu.py.
    m.def("_merge_states", &mha_merge_states, "Merge partial attention states (O_i, LSE_i) into one (O, LSE)",
          py::arg("o_parts"), py::arg("lse_parts"), py::arg("sink") = py::none(), py::arg("packed") = false,
          py::arg("out") = py::none(), py::arg("lse_out") = py::none());
    // `mla_decode` likewise: bound as `_mla_decode`, reached as `paged_attn.mla_decode`
    m.def("_mla_decode", &mha_mla_decode<false>, "MLA decode over a paged latent KV cache (d_qk 576, d_v 512)",
          py::arg("q"), py::arg("kv_cache"), py::arg("block_table"), py::arg("cache_seqlens"),
          py::arg("head_dim_v") = 512, py::arg("softmax_scale") = 0.041666666666666664f,
          py::arg("is_causal") = false, py::arg("num_splits") = 0, py::arg("out") = py::none());
    // ... and its fp8-cache twin and the append into that cache, reached the same way
    m.def("_mla_decode_fp8", &mha_mla_decode<true>, "MLA decode over an fp8 paged latent KV cache (rows of 656 bytes)",
          py::arg("q"), py::arg("kv_cache"), py::arg("block_table"), py::arg("cache_seqlens"),
          py::arg("head_dim_v") = 512, py::arg("softmax_scale") = 0.041666666666666664f,
          py::arg("is_causal") = false, py::arg("num_splits") = 0, py::arg("out") = py::none());
    m.def("_mla_cache_append_fp8", &mha_mla_cache_append_fp8, "Append tokens to an fp8 paged latent KV cache",
          py::arg("latent"), py::arg("k_pe"), py::arg("kv_cache"), py::arg("slot_mapping"));
    // ... and the two decodes over index-selected tokens
    m.def("_mla_decode_sparse", &mha_mla_decode_sparse<false>, "MLA decode over index-selected tokens of a paged latent KV cache",
          py::arg("q"), py::arg("kv_cache"), py::arg("indices"), py::arg("head_dim_v") = 512,
          py::arg("softmax_scale") = 0.041666666666666664f, py::arg("num_splits") = 0, py::arg("out") = py::none());
    m.def("_mla_decode_sparse_fp8", &mha_mla_decode_sparse<true>, "MLA decode over index-selected tokens of an fp8 paged latent KV cache",
          py::arg("q"), py::arg("kv_cache"), py::arg("indices"), py::arg("head_dim_v") = 512,
          py::arg("softmax_scale") = 0.041666666666666664f, py::arg("num_splits") = 0, py::arg("out") = py::none());
    // ... and the MLA prefill (head size 192 for q / k, 128 for v), dense and packed
    m.def("_fwd_mla", &mha_fwd_mla, "MLA prefill forward (d_qk 192, d_v 128)", py::arg("q"), py::arg("k"),
          py::arg("v"), py::arg("out") = py::none(), py::arg("softmax_scale") = 0.07216878364870322f,
          py::arg("is_causal") = false, py::arg("window_size_left") = -1, py::arg("window_size_right") = -1);
    m.def("_varlen_fwd_mla", &mha_varlen_fwd_mla, "MLA prefill forward over packed sequences (d_qk 192, d_v 128)",
          py::arg("q"), py::arg("k"), py::arg("v"), py::arg("out"), py::arg("cu_seqlens_q"),
          py::arg("cu_seqlens_k"), py::arg("seqused_k"), py::arg("max_seqlen_q"), py::arg("max_seqlen_k"),
          py::arg("softmax_scale") = 0.07216878364870322f, py::arg("is_causal") = false,
          py::arg("window_size_left") = -1, py::arg("window_size_right") = -1);
    // ... and its backward
    m.def("_bwd_mla", &mha_bwd_mla, "MLA prefill backward (d_qk 192, d_v 128)", py::arg("dout"), py::arg("q"),
          py::arg("k"), py::arg("v"), py::arg("out"), py::arg("softmax_lse"), py::arg("dq") = py::none(),
          py::arg("dk") = py::none(), py::arg("dv") = py::none(), py::arg("softmax_scale") = 0.07216878364870322f,
          py::arg("is_causal") = false, py::arg("window_size_left") = -1, py::arg("window_size_right") = -1);
    m.def("_varlen_bwd_mla", &mha_varlen_bwd_mla, "MLA prefill backward over packed sequences (d_qk 192, d_v 128)",
          py::arg("dout"), py::arg("q"), py::arg("k"), py::arg("v"), py::arg("out"), py::arg("softmax_lse"),
          py::arg("dq"), py::arg("dk"), py::arg("dv"), py::arg("cu_seqlens_q"), py::arg("cu_seqlens_k"),
          py::arg("max_seqlen_q"), py::arg("max_seqlen_k"), py::arg("softmax_scale") = 0.07216878364870322f,
          py::arg("is_causal") = false, py::arg("window_size_left") = -1, py::arg("window_size_right") = -1);
    const py::handle self = m;
    m.def("__getattr__", [self](const std::string& name) -> py::object {
        if (name == "merge_states") return self.attr("_merge_states");
        if (name == "mla_decode") return self.attr("_mla_decode");
        if (name == "mla_decode_fp8") return self.attr("_mla_decode_fp8");
        if (name == "mla_cache_append_fp8") return self.attr("_mla_cache_append_fp8");
        if (name == "mla_decode_sparse") return self.attr("_mla_decode_sparse");
        if (name == "mla_decode_sparse_fp8") return self.attr("_mla_decode_sparse_fp8");
        if (name == "fwd_mla") return self.attr("_fwd_mla");
        if (name == "varlen_fwd_mla") return self.attr("_varlen_fwd_mla");
        if (name == "bwd_mla") return self.attr("_bwd_mla");
        if (name == "varlen_bwd_mla") return self.attr("_varlen_bwd_mla");
        PyErr_SetString(PyExc_AttributeError, ("module 'paged_attn' has no attribute '" + name + "'").c_str());
        throw py::error_already_set();
    });
    m.def("version",[]() { return std::string(fmha_version()); });
}
