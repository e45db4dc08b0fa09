"""GPU: one-defect calls of `paged_attn.merge_states`, in the style (and with the helpers) of
tests/test_ops_validation_gpu.py: an otherwise valid small call, one argument broken, RuntimeError
and a substring of the message pinned.  Every row is refused by the binding's checks or by the C
entry's, before a kernel is launched.

`merge_states` is reached by name through the module's __getattr__ and is not in dir(paged_attn),
the listed table of attention ops that tests/test_ops_validation_gpu.py covers; this file is its
table."""
import pytest

from tests.test_ops_validation_gpu import B, BF, D, F16, F32, H, S, _cols, _heads, _t, new, put

pytestmark = pytest.mark.gpu


def _merge_states(d=D, dtype=BF, packed=False, n=2):
    o = (B * S, H, d) if packed else (B, S, H, d)
    lse = (H, B * S) if packed else (B, H, S)
    return dict(o_parts=[_t(*o, dtype=dtype) for _ in range(n)], lse_parts=[_t(*lse, dtype=F32) for _ in range(n)],
                sink=None, packed=packed, out=None, lse_out=None)


def each(name, f):
    return lambda a: {name: [f(t) for t in a[name]]}


def second(name, f):
    return lambda a: {name: [a[name][0], f(a[name][1])]}


ROWS = [
    (dict(n=17), put(), "merge_states takes 1 to 16 parts"),
    ({}, lambda a: {"lse_parts": a["lse_parts"] * 2}, "o_parts and lse_parts must have the same length"),
    (dict(dtype=F32), put(), "o_parts must be fp16 or bf16"),
    ({}, each("lse_parts", lambda t: t.to(BF)), "lse_parts must have dtype fp32"),
    ({}, second("o_parts", lambda t: t.to(F16)), "o_parts must share one dtype"),
    ({}, second("o_parts", lambda t: t[:, 1:]), "o_parts must share one shape"),
    ({}, second("o_parts", _heads), "o_parts must share one stride set"),
    ({}, second("lse_parts", lambda t: _heads(t[..., None])[..., 0]), "lse_parts must share one stride set"),
    ({}, each("o_parts", _cols), "o_parts must have contiguous last dimension"),
    ({}, each("o_parts", lambda t: t.cpu()), "must be on one CUDA device"),
    ({}, each("lse_parts", lambda t: t.cpu()), "must be on one CUDA device"),
    ({}, each("o_parts", lambda t: t[0]), "o_parts must be (batch, seqlen, heads, head_size)"),
    (dict(packed=True), each("o_parts", lambda t: t[None]), "o_parts must be (total, heads, head_size)"),
    ({}, each("lse_parts", lambda t: t[0]), "lse_parts must be (batch, heads, rows)"),
    ({}, each("lse_parts", lambda t: t.transpose(1, 2).contiguous()), "must have shape"),
    (dict(d=60), put(), "head_size must be a multiple of 8 and at most 256"),
    (dict(d=264), put(), "head_size must be a multiple of 8 and at most 256"),
    ({}, new("sink", H + 1, dtype=F32), "sink must have shape (num_heads)"),
    ({}, new("sink", H), "sink must have dtype fp32"),
    ({}, new("out", B, S, H, D, dtype=F16), "out must have the dtype of the parts"),
    ({}, new("out", B, S, H, D + 8), "out must have the shape of the parts"),
    ({}, lambda a: {"out": _t(B, S, H, D).cpu()}, "out must be on the parts' device"),
    ({}, lambda a: {"out": _cols(_t(B, S, H, D))}, "out must have contiguous last dimension"),
    ({}, new("lse_out", B, H, S, dtype=BF), "lse_out must have the dtype of the parts"),
    ({}, new("lse_out", B, H, S + 1, dtype=F32), "lse_out must have the shape of the parts"),
    ({}, lambda a: {"out": a["o_parts"][1]}, "o overlaps part 1"),
    ({}, lambda a: {"lse_out": a["lse_parts"][1]}, "lse overlaps part 1"),
]


@pytest.mark.parametrize("base_kw,defect,needle", ROWS, ids=[f"merge_states-{i}" for i in range(len(ROWS))])
def test_one_defect_is_refused(base_kw, defect, needle):
    from xf_flash_attention_cutlass_amd import paged_attn
    a = _merge_states(**base_kw)
    over = defect(a)
    assert set(over) <= set(a), sorted(over)
    a.update(over)
    with pytest.raises(RuntimeError) as e:
        paged_attn.merge_states(*a.values())
    assert type(e.value) is RuntimeError, type(e.value)      # not one of its subclasses
    assert needle in str(e.value)


def test_valid_call_and_name_resolution():
    """the unbroken call of the table runs, `merge_states` resolves to the bound function, and an
    unknown name is still an AttributeError"""
    from xf_flash_attention_cutlass_amd import paged_attn
    out, lse = paged_attn.merge_states(*_merge_states().values())
    assert out.shape == (B, S, H, D) and lse.shape == (B, H, S)
    assert paged_attn.merge_states is paged_attn._merge_states
    assert "merge_states" not in dir(paged_attn) and not hasattr(paged_attn, "no_such_op")
