"""CPU: one-defect calls through fake pointers for every compute entry of the C ABI.  Each row
breaks one argument of an otherwise valid call and pins the status (1: refused before anything
is allocated or launched) and a substring of the message.  No kernel is launched here."""
import ctypes

import pytest

from xf_flash_attention_cutlass_amd import capi

FAKE = 0x1000          # 16-byte aligned, never dereferenced
BIG = 1 << 40          # a caller's workspace that always fits (no pool allocation)


def _strides(b=2, sq=16, sk=16, h=4, hk=2, d=64):
    q = [sq * h * d, h * d, d]
    k = [sk * hk * d, hk * d, d]
    return q + k + k + q


# entry -> (exported function, a valid call's arguments in the C order)
ENTRIES = {
    "fwd": ("fmha_fwd", dict(
        q=FAKE, k=FAKE, v=FAKE, o=FAKE, alibi=None, sq=16, sk=16, b=2, h=4, hk=2, d=64, p=0.0,
        stream=None, dprops=None, scale=0.125, p_ptr=None, lse=None, wl=-1, wr=-1, softcap=0.0,
        ret=False, fp16=False, splits=1)),
    "strided": ("fmha_fwd_strided", dict(
        q=FAKE, k=FAKE, v=FAKE, o=FAKE, alibi=None, lse=None, sq=16, sk=16, b=2, h=4, hk=2, d=64,
        st=_strides(), scale=0.125, wl=-1, wr=-1, softcap=0.0, fp16=False, splits=1, stream=None,
        p=0.0, s_dmask=None)),
    "fp8": ("fmha_fwd_fp8", dict(
        q=FAKE, k=FAKE, v=FAKE, o=FAKE, lse=None, qs=1.0, ks=1.0, vs=1.0, sq=16, sk=16, b=2, h=4,
        hk=2, d=128, scale=0.088, wl=-1, wr=-1, fp16=False, stream=None)),
    "varlen_fp8": ("fmha_varlen_fwd_fp8", dict(
        q=FAKE, k=FAKE, v=FAKE, o=FAKE, lse=None, cu_q=FAKE, cu_k=FAKE, seqused=None, qs=1.0,
        ks=1.0, vs=1.0, max_q=16, max_k=16, total_q=32, b=2, h=4, hk=2, d=128, scale=0.088,
        wl=-1, wr=-1, fp16=False, stream=None)),
    "varlen_ex": ("fmha_varlen_fwd_ex", dict(
        q=FAKE, k=FAKE, v=FAKE, o=FAKE, lse=None, cu_q=FAKE, cu_k=FAKE, seqused=None, bt=None,
        bt_stride=0, page=0, alibi=None, alibi_bs=0, max_q=16, max_k=16, total_q=32, b=2, h=4,
        hk=2, d=64, scale=0.125, wl=-1, wr=-1, softcap=0.0, fp16=False, stream=None, p=0.0,
        s_dmask=None)),
    "varlen": ("fmha_varlen_fwd", dict(
        q=FAKE, k=FAKE, v=FAKE, o=FAKE, cu_q=FAKE, cu_k=FAKE, max_q=16, max_k=16, b=2, h=4, hk=2,
        d=64, stream=None, scale=0.125, causal=False, fp16=False, wl=-1, wr=-1)),
    "paged_ex": ("fmha_page_kvcache_fwd_ex", dict(
        q=FAKE, k=FAKE, v=FAKE, o=FAKE, lse=None, bt=FAKE, bt_stride=4, seqlens=FAKE, sq=1,
        max_k=64, b=2, h=4, hk=2, d=64, page=16, scale=0.125, wl=-1, wr=-1, softcap=0.0,
        alibi=None, alibi_bs=0, splits=1, kv_dtype=0, ks=1.0, vs=1.0, leftpad=None, fp16=False,
        stream=None)),
    "paged": ("fmha_page_kvcache_fwd", dict(
        q=FAKE, k=FAKE, v=FAKE, knew=None, vnew=None, o=FAKE, bt=FAKE, seqlens=FAKE, max_cache=64,
        sq=1, sk=64, b=2, h=4, hk=2, d=64, page=16, stream=None, scale=0.125, wl=-1, wr=-1,
        splits=1, batch_idx=None, cos=None, sin=None, causal=False, interleaved=False,
        fp16=False)),
    "append": ("fmha_kvcache_append", dict(
        q=None, q_out=None, kc=FAKE, vc=FAKE, knew=FAKE, vnew=FAKE, snew=1, bt=FAKE, bt_stride=4,
        page=16, seqlens=FAKE, seqlens_out=FAKE + 64, cos=None, sin=None, rdim=0,
        interleaved=False, per_token=False, b=2, sq=1, h=4, hk=2, d=64, fp16=False, stream=None)),
    "bwd": ("fmha_bwd", dict(
        dout=FAKE, q=FAKE, k=FAKE, v=FAKE, o=FAKE, lse=FAKE, dq=FAKE, dk=FAKE, dv=FAKE,
        alibi=None, softmax_d=None, sq=16, sk=16, b=2, h=4, hk=2, d=64, p=0.0, scale=0.125,
        wl=-1, wr=-1, softcap=0.0, det=False, fp16=False, stream=None, ws=FAKE, ws_bytes=BIG)),
    "varlen_bwd": ("fmha_varlen_bwd", dict(
        dout=FAKE, q=FAKE, k=FAKE, v=FAKE, o=FAKE, lse=FAKE, dq=FAKE, dk=FAKE, dv=FAKE,
        cu_q=FAKE, cu_k=FAKE, alibi=None, alibi_bs=0, max_q=16, max_k=16, total_q=32, total_k=32,
        b=2, h=4, hk=2, d=64, scale=0.125, wl=-1, wr=-1, softcap=0.0, det=False, fp16=False,
        stream=None, ws=FAKE, ws_bytes=BIG, softmax_d=None, p=0.0)),
}

# the checks every entry with q / k / v / o shares (check_common)
COMMON = [
    (dict(q=None), "non-null"),
    (dict(v=None), "non-null"),
    (dict(k=FAKE + 2), "16-byte aligned"),
    (dict(o=FAKE + 8), "16-byte aligned"),
    (dict(b=0), "batch size must be positive"),
    (dict(h=3, hk=2), "must divide"),
    (dict(hk=0), "must divide"),
    (dict(d=60), "multiple of 8"),
    (dict(d=0), "multiple of 8"),
    (dict(d=264), "at most 256"),
]
COMMON_ENTRIES = ("fwd", "strided", "fp8", "varlen_fp8", "varlen_ex", "varlen", "paged_ex",
                  "paged", "bwd", "varlen_bwd")

SLAB = "32-bit offsets"
ROWS = [
    # ---- fmha_fwd
    ("fwd", dict(sq=0), "seqlen_q/seqlen_k must be positive"),
    ("fwd", dict(sk=-1), "seqlen_q/seqlen_k must be positive"),
    ("fwd", dict(p=1.0), "p_dropout must be in [0, 1)"),
    ("fwd", dict(p=-0.1), "p_dropout must be in [0, 1)"),
    ("fwd", dict(p=0.1, softcap=30.0), "Softcapping does not support dropout"),
    ("fwd", dict(ret=True), "return_softmax is only supported when p_dropout > 0.0"),
    ("fwd", dict(ret=True, p=0.1), "return_softmax needs the p and softmax_lse buffers"),
    ("fwd", dict(sq=1 << 24, h=64, hk=64, d=128), "q/o: one sequence spans"),
    ("fwd", dict(sk=1 << 24, h=64, hk=64, d=128), "k/v: one sequence spans"),
    # ---- fmha_fwd_strided
    ("strided", dict(st=None), "strides must be non-null"),
    ("strided", dict(sq=0), "seqlen_q/seqlen_k must be positive"),
    ("strided", dict(st=[-8] + _strides()[1:]), "strides must be non-negative"),
    ("strided", dict(st=_strides()[:4] + [132] + _strides()[5:]), "multiples of 8 elements (16 bytes): stride 4"),
    ("strided", dict(s_dmask=FAKE), "s_dmask needs p_dropout > 0 and softmax_lse"),
    ("strided", dict(s_dmask=FAKE, p=0.1), "s_dmask needs p_dropout > 0 and softmax_lse"),
    ("strided", dict(p=1.0), "p_dropout must be in [0, 1)"),
    ("strided", dict(p=0.1, softcap=30.0), "Softcapping does not support dropout"),
    ("strided", dict(st=_strides()[:1] + [1 << 31] + _strides()[2:]), "q: one sequence spans"),
    ("strided", dict(st=_strides()[:4] + [1 << 31] + _strides()[5:]), "k: one sequence spans"),
    ("strided", dict(st=_strides()[:7] + [1 << 31] + _strides()[8:]), "v: one sequence spans"),
    ("strided", dict(st=_strides()[:10] + [1 << 31] + _strides()[11:]), "o: one sequence spans"),
    # ---- fmha_fwd_fp8
    ("fp8", dict(d=64), "the fp8 forward supports head_size 128"),
    ("fp8", dict(sq=0), "seqlen_q/seqlen_k must be positive"),
    ("fp8", dict(sk=0), "seqlen_q/seqlen_k must be positive"),
    ("fp8", dict(qs=0.0), "fp8 descales must be positive"),
    ("fp8", dict(ks=-1.0), "fp8 descales must be positive"),
    ("fp8", dict(vs=0.0), "fp8 descales must be positive"),
    ("fp8", dict(sq=1 << 24, h=64, hk=64), "q: one sequence spans"),
    ("fp8", dict(sk=1 << 24, h=64, hk=64), "k/v: one sequence spans"),
    ("fp8", dict(sq=1 << 20, h=8, hk=1), "o: one sequence spans"),      # q (1 byte) fits, o does not
    # ---- fmha_varlen_fwd_fp8
    ("varlen_fp8", dict(cu_q=None), "cu_seqlens_q and cu_seqlens_k must be given"),
    ("varlen_fp8", dict(cu_k=None), "cu_seqlens_q and cu_seqlens_k must be given"),
    ("varlen_fp8", dict(d=64), "the fp8 forward supports head_size 128"),
    ("varlen_fp8", dict(qs=0.0), "fp8 descales must be positive"),
    ("varlen_fp8", dict(vs=-1.0), "fp8 descales must be positive"),
    ("varlen_fp8", dict(max_q=0), "max_seqlen_q must be positive"),
    ("varlen_fp8", dict(max_k=0), "max_seqlen_k must be positive"),
    ("varlen_fp8", dict(lse=FAKE, total_q=0), "total_q must be given to address the LSE"),
    ("varlen_fp8", dict(max_q=1 << 24, h=64, hk=64), "q: one sequence spans"),
    ("varlen_fp8", dict(max_k=1 << 24, h=64, hk=64), "k/v: one sequence spans"),
    ("varlen_fp8", dict(max_q=1 << 20, h=8, hk=1), "o: one sequence spans"),
    ("varlen_fp8", dict(lse=FAKE, total_q=1 << 29), "softmax_lse: one sequence spans"),
    # ---- fmha_varlen_fwd_ex
    ("varlen_ex", dict(cu_q=None), "cu_seqlens_q and cu_seqlens_k (or a block table) must be given"),
    ("varlen_ex", dict(cu_k=None), "cu_seqlens_q and cu_seqlens_k (or a block table) must be given"),
    ("varlen_ex", dict(max_q=0), "max_seqlen_q must be positive"),
    ("varlen_ex", dict(max_k=0), "max_seqlen_k == 0: nothing to attend to"),
    ("varlen_ex", dict(bt=FAKE, bt_stride=4, page=0, seqused=FAKE), "page_block_size must be positive"),
    ("varlen_ex", dict(bt=FAKE, bt_stride=4, page=16, cu_k=None), "paged varlen needs seqused_k or cu_seqlens_k"),
    ("varlen_ex", dict(lse=FAKE, total_q=0), "total_q must be given to address the LSE"),
    ("varlen_ex", dict(s_dmask=FAKE, lse=FAKE), "s_dmask needs p_dropout > 0"),
    ("varlen_ex", dict(s_dmask=FAKE, lse=FAKE, p=0.1, bt=FAKE, bt_stride=4, page=16), "s_dmask needs p_dropout > 0"),
    ("varlen_ex", dict(p=0.1, bt=FAKE, bt_stride=4, page=16), "dropout over a paged K/V cache is not supported"),
    ("varlen_ex", dict(p=1.0), "p_dropout must be in [0, 1)"),
    ("varlen_ex", dict(p=0.1, softcap=30.0), "Softcapping does not support dropout"),
    ("varlen_ex", dict(max_q=1 << 24, h=64, hk=64, d=128), "q/o: one sequence spans"),
    ("varlen_ex", dict(max_k=1 << 24, h=64, hk=64, d=128), "k/v: one sequence spans"),
    # ---- fmha_varlen_fwd (the reference's entry: forwards to the _ex one)
    ("varlen", dict(cu_q=None), "cu_seqlens_q and cu_seqlens_k (or a block table) must be given"),
    ("varlen", dict(max_k=0), "nothing to attend to"),
    # ---- fmha_page_kvcache_fwd_ex
    ("paged_ex", dict(bt=None), "block_table must be given for the paged KV path"),
    ("paged_ex", dict(page=0), "page_block_size must be positive"),
    ("paged_ex", dict(page=-16), "page_block_size must be positive"),
    ("paged_ex", dict(sq=0), "seqlen_q / seqlen_k must be positive"),
    ("paged_ex", dict(max_k=0), "seqlen_q / seqlen_k must be positive"),
    ("paged_ex", dict(kv_dtype=2), "kv_dtype must be 0 (same as q) or 1 (fp8 e4m3fn)"),
    ("paged_ex", dict(kv_dtype=-1), "kv_dtype must be 0 (same as q) or 1 (fp8 e4m3fn)"),
    ("paged_ex", dict(bt_stride=0), "block_table_stride must be positive"),
    ("paged_ex", dict(bt_stride=-4), "block_table_stride must be positive"),
    ("paged_ex", dict(leftpad=FAKE), "Paged KV and leftpad_k are not supported at the same time"),
    ("paged_ex", dict(sq=1 << 24, h=64, hk=64, d=128), "q/o: one sequence spans"),
    ("paged_ex", dict(page=1 << 20, max_k=1 << 20, h=64, hk=64, d=128), "kcache/vcache page: one sequence spans"),
    # ---- fmha_page_kvcache_fwd (the reference's entry)
    ("paged", dict(page=0), "page_block_size must be positive"),
    ("paged", dict(bt=None), "block_table must be given"),
    # ---- fmha_kvcache_append
    ("append", dict(kc=None), "kcache, vcache, block_table and cache_seqlens must be given"),
    ("append", dict(snew=-1), "seqlen_new must be >= 0"),
    ("append", dict(vnew=None), "new K and V must both be given"),
    ("append", dict(h=3), "invalid batch / head counts"),
    ("append", dict(d=60), "head_size must be a multiple of 8"),
    ("append", dict(page=0), "page_block_size must be positive"),
    ("append", dict(bt_stride=0), "block_table_stride must be positive"),
    ("append", dict(seqlens_out=FAKE), "seqlens_out must not alias cache_seqlens"),
    ("append", dict(rdim=24), "Only rotary dimensions divisible by 16"),
    ("append", dict(rdim=16), "rotary needs cos, sin, q and q_out"),
    # ---- fmha_bwd
    ("bwd", dict(dout=None), "dout/softmax_lse/dq/dk/dv must be non-null"),
    ("bwd", dict(lse=None), "dout/softmax_lse/dq/dk/dv must be non-null"),
    ("bwd", dict(dv=None), "dout/softmax_lse/dq/dk/dv must be non-null"),
    ("bwd", dict(p=0.1, softcap=30.0), "Softcapping does not support dropout"),
    ("bwd", dict(sq=0), "seqlen_q/seqlen_k must be positive"),
    ("bwd", dict(sk=0), "seqlen_q/seqlen_k must be positive"),
    ("bwd", dict(p=1.0), "p_dropout must be in [0, 1)"),
    ("bwd", dict(p=-0.5), "p_dropout must be in [0, 1)"),
    ("bwd", dict(ws_bytes=16), "workspace too small"),
    ("bwd", dict(ws_bytes=16, det=True), "workspace too small"),
    ("bwd", dict(sq=1 << 24, h=64, hk=64, d=128), "q/out/dout/dq: one sequence spans"),
    ("bwd", dict(sk=1 << 24, h=64, hk=64, d=128), "k/v/dk/dv: one sequence spans"),
    ("bwd", dict(sq=1 << 22, h=1, hk=1, d=128), "dq_accum: one sequence spans"),
    ("bwd", dict(sq=1 << 16, b=1 << 11, h=8, hk=8, d=128), "rows exceed the 32-bit thread index"),
    # ---- fmha_varlen_bwd
    ("varlen_bwd", dict(dq=None), "dout/softmax_lse/dq/dk/dv must be non-null"),
    ("varlen_bwd", dict(p=0.1, softcap=30.0), "Softcapping does not support dropout"),
    ("varlen_bwd", dict(cu_q=None), "cu_seqlens_q/cu_seqlens_k must be non-null"),
    ("varlen_bwd", dict(cu_k=None), "cu_seqlens_q/cu_seqlens_k must be non-null"),
    ("varlen_bwd", dict(total_q=0), "total/max sequence lengths must be positive"),
    ("varlen_bwd", dict(total_k=0), "total/max sequence lengths must be positive"),
    ("varlen_bwd", dict(max_q=0), "total/max sequence lengths must be positive"),
    ("varlen_bwd", dict(max_k=-1), "total/max sequence lengths must be positive"),
    ("varlen_bwd", dict(p=1.0), "p_dropout must be in [0, 1)"),
    ("varlen_bwd", dict(ws_bytes=16), "workspace too small"),
    ("varlen_bwd", dict(ws_bytes=16, det=True), "workspace too small"),
    ("varlen_bwd", dict(max_q=1 << 24, total_q=1 << 24, h=64, hk=64, d=128), "q/out/dout/dq: one sequence spans"),
    ("varlen_bwd", dict(max_k=1 << 24, total_k=1 << 24, h=64, hk=64, d=128), "k/v/dk/dv: one sequence spans"),
    ("varlen_bwd", dict(max_q=1 << 22, total_q=1 << 22, h=1, hk=1, d=128), "dq_accum: one sequence spans"),
    ("varlen_bwd", dict(max_q=1 << 16, total_q=1 << 27, h=8, hk=8, d=128), "rows exceed the 32-bit thread index"),
]
ROWS += [(e, over, needle) for e in COMMON_ENTRIES for over, needle in COMMON]


def _call(entry, over):
    fn, base = ENTRIES[entry]
    a = dict(base)
    assert set(over) <= set(a), (entry, over)
    a.update(over)
    if isinstance(a.get("st"), list):
        a["st"] = (ctypes.c_int64 * 12)(*a["st"])
    L = capi.lib()
    getattr(L, fn)(*a.values())
    return L.fmha_last_status(), L.fmha_last_error().decode()


@pytest.mark.parametrize("entry,over,needle", ROWS,
                         ids=[f"{e}-{'-'.join(o)}-{i}" for i, (e, o, _) in enumerate(ROWS)])
def test_one_defect_is_refused(entry, over, needle):
    status, msg = _call(entry, over)
    assert status == 1, (status, msg)
    assert needle in msg, msg
    if entry not in ("append", "bwd", "varlen_bwd"):
        L = capi.lib()                         # a refused forward launched nothing
        assert L.fmha_last_kernel().decode() == "" and L.fmha_last_num_splits() == 0


def test_slab_rows_name_the_limit():
    for entry, over, needle in ROWS:
        if "one sequence spans" in needle:
            assert SLAB in _call(entry, over)[1]


# ------------------------------------------------------------------------------- knobs ----
# name, default, lo, hi (fmha_launch.h)
KNOBS = [
    ("fwd_w4", 4, 0, 4), ("fp8_w4", 1, 0, 2), ("fwd_waves", 8, 4, 8), ("fwd_prio", 0, 0, 1),
    ("fwd_persistent", 1, 0, 8), ("fwd_slack", 8, 0, 16), ("fwd_order", 1, 0, 1),
    ("fwd_dyn", 1, 0, 2), ("fwd_xcdq", 1, 0, 1), ("fwd_pipe", 1, 0, 2), ("fwd_decode", 1, 0, 1),
    ("dec_wg_per_cu", 2, 1, 16), ("dec_mr", 16, 16, 32), ("comb_row", 1, 0, 1),
    ("dec_fold", 0, 0, 1), ("dec_bal", 1, 0, 1), ("bwd_order", 0, 0, 1), ("bwd_desc", 1, 0, 1),
    ("dec_hmaj", 1, 0, 2),
]
VARIANTS_ONLY = {"fwd_w4": 1, "fp8_w4": 2}     # values the product build refuses


@pytest.fixture(scope="module")
def private_libs(tmp_path_factory):
    """Own copies of the product and the variants library: a copy under another path is a
    separate load with its own option state, so these tests neither see nor disturb the knobs
    the rest of the session runs under (XFA_TEST_OPTIONS)."""
    import shutil
    d = tmp_path_factory.mktemp("knobs")
    out = []
    for i, path in enumerate((capi.LIB_PATH, capi.VARIANTS_PATH)):
        dst = d / f"knobs{i}.so"
        shutil.copy(path, dst)
        out.append(capi.load(str(dst)))
    return out


@pytest.mark.parametrize("name,default,lo,hi", KNOBS)
def test_knob_default_range_and_round_trip(private_libs, name, default, lo, hi):
    key = name.encode()
    for which, L in enumerate(private_libs):
        assert L.fmha_get_option(key) == default and L.fmha_last_status() == 0
        for bad in (lo - 1, hi + 1):
            assert L.fmha_set_option(key, bad) == -1
            assert L.fmha_last_status() == 1
            assert f"option {name}: value {bad} out of range [{lo}, {hi}]" in L.fmha_last_error().decode()
            assert L.fmha_get_option(key) == default
        for val in (lo, hi):
            if which == 0 and VARIANTS_ONLY.get(name) == val:
                continue                       # (test_variants_only_values)
            assert L.fmha_set_option(key, val) == 0 and L.fmha_last_status() == 0
            assert L.fmha_get_option(key) == val
        assert L.fmha_set_option(key, default) == 0


@pytest.mark.parametrize("name,good,bad", [("fwd_waves", (4, 8), (5, 6, 7)),
                                           ("dec_mr", (16, 32), (17, 24, 31))])
def test_enumerated_knobs(private_libs, name, good, bad):
    L = private_libs[0]
    key = name.encode()
    default = L.fmha_get_option(key)
    for val in bad:
        assert L.fmha_set_option(key, val) == -1 and L.fmha_last_status() == 1
        assert "out of range" in L.fmha_last_error().decode()
        assert L.fmha_get_option(key) == default
    for val in good:
        assert L.fmha_set_option(key, val) == 0 and L.fmha_get_option(key) == val
    assert L.fmha_set_option(key, default) == 0


@pytest.mark.parametrize("name,val", sorted(VARIANTS_ONLY.items()))
def test_variants_only_values(private_libs, name, val):
    product, variants = private_libs
    key = name.encode()
    default = product.fmha_get_option(key)
    assert product.fmha_set_option(key, val) == -1 and product.fmha_last_status() == 1
    assert "only the variants build has" in product.fmha_last_error().decode()
    assert product.fmha_get_option(key) == default
    assert variants.fmha_set_option(key, val) == 0 and variants.fmha_get_option(key) == val
    assert variants.fmha_set_option(key, default) == 0


def test_unknown_and_null_knob_names(private_libs):
    L = private_libs[0]
    assert L.fmha_set_option(b"no_such_knob", 1) == -1 and L.fmha_last_status() == 1
    assert "unknown option 'no_such_knob'" in L.fmha_last_error().decode()
    assert L.fmha_get_option(b"no_such_knob") == -1 and L.fmha_last_status() == 1
    assert "unknown option 'no_such_knob'" in L.fmha_last_error().decode()
    assert L.fmha_set_option(None, 1) == -1 and "option name is null" in L.fmha_last_error().decode()
    assert L.fmha_get_option(None) == -1 and "option name is null" in L.fmha_last_error().decode()
    assert L.fmha_get_option(b"fwd_dyn") == 1 and L.fmha_last_status() == 0   # and the error is cleared
