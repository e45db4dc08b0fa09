"""CPU: the plain body tools/gen_fwdpp.py emits (fwdpp_plain_item_*, fmha_fwdpp_body_plain.h, which
build.py generates before it compiles: the header is not committed) — the header the build
compiles is the generator's default output, its text names no feature / left-window
operand, its inline unmasked step is shorter than the full body's, and each of its two reduction
options (lazy_lim, max0) changes only the instructions it names."""
import difflib
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "xf_flash_attention_cutlass_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "tools"))


def _functions(path):
    """{function name: [instruction / label lines]} of a generated header"""
    out = {}
    for m in re.finditer(r"(?s)void (\w+)\((.*?)\) \{\n    asm volatile\(\n(.*?)\n        :", open(path).read()):
        out[m.group(1)] = [ln.strip()[1:-3] for ln in m.group(3).splitlines()]      # "text\n"
    return out


@pytest.fixture(scope="module")
def bodies(tmp_path_factory):
    import gen_fwdpp
    d = tmp_path_factory.mktemp("plain")
    out = {}
    for tag, opts in (("default", {}), ("nolazy", dict(lazy_lim=False)), ("nomax0", dict(max0=False))):
        path = str(d / f"{tag}.h")
        gen_fwdpp.emit(path, **opts)
        out[tag] = (path, gen_fwdpp.plain_path(path))
    return out


def test_built_plain_header_matches_generator(bodies):
    import importlib.util
    spec = importlib.util.spec_from_file_location(
        "_xfa_build", os.path.join(ROOT, "xf_flash_attention_cutlass_amd", "build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)
    full, plain = bodies["default"]
    built = build.generate()                   # (rewrites nothing when it is up to date)
    assert os.path.dirname(built) == build.GEN and build.GEN in build.HIP_FLAGS
    assert open(plain, "rb").read() == open(built, "rb").read()
    assert not os.path.exists(os.path.join(CSRC, "fmha_fwdpp_body_plain.h"))   # (one copy: the build's)
    assert open(full, "rb").read() == open(os.path.join(CSRC, "fmha_fwdpp_body.h"), "rb").read()
    # the options are the plain body's alone
    for tag in ("nolazy", "nomax0"):
        assert open(bodies[tag][0], "rb").read() == open(full, "rb").read()


def test_plain_functions_name_no_feature_operand(bodies):
    text = open(bodies["default"][1]).read()
    fns = _functions(bodies["default"][1])
    assert sorted(fns) == ["fwdpp_plain_item_bf16", "fwdpp_plain_item_f16"]
    for op in "feat fw lw liml wid alw ald alm scp2 alw2 adiag".split():
        assert f"%[{op}]" not in text and f" {op}," not in text and f" {op})" not in text, op
    # registers 96-99 (LIML, its temp, SHIFT, NMTRUE) are neither used nor clobbered
    assert not re.search(r"\bv9[6-9]\b", text)


def _step(lines, grp="A", ph=0):
    """the inline step of ring phase ph: from its selector to the next phase's label"""
    a = lines.index(f".Lph{ph}_{grp}_%=:")
    b = lines.index(f".Lnx{ph}_{grp}_%=:")
    return lines[a:b]


def _count(lines, prefix):
    return sum(ln.startswith(prefix) and not ln.startswith(("v_mfma", "s_nop", "s_waitcnt", "s_barrier"))
               for ln in lines)


def test_unmasked_step_is_shorter(bodies):
    full = _functions(bodies["default"][0])["fwdpp_item_bf16"]
    for tag in ("default", "nolazy"):
        plain = _functions(bodies[tag][1])["fwdpp_plain_item_bf16"]
        for grp in "AB":
            for ph in range(4):
                f, p = _step(full, grp, ph), _step(plain, grp, ph)
                assert _count(p, "v_") < _count(f, "v_") and _count(p, "s_") < _count(f, "s_"), (tag, grp, ph)
                assert _count(p, "v_mfma") == _count(f, "v_mfma") == 0       # (counted apart)
                assert sum(ln.startswith("v_mfma") for ln in p) == sum(ln.startswith("v_mfma") for ln in f) == 32
                assert sum(ln.startswith("ds_read") for ln in p) == sum(ln.startswith("ds_read") for ln in f)
    # the default plain step against the full one: LIML's and LIM's adds (2 VALU); the feature
    # test and the two left-window selector compares, each with its branch (6 SALU)
    f, p = _step(full), _step(_functions(bodies["default"][1])["fwdpp_plain_item_bf16"])
    assert _count(f, "v_") - _count(p, "v_") == 2 and _count(f, "s_") - _count(p, "s_") == 6


def _changed(a, b):
    """(lines only in a, lines only in b) of two instruction lists"""
    only_a, only_b = [], []
    for ln in difflib.ndiff(a, b):
        if ln.startswith("- "):
            only_a.append(ln[2:])
        elif ln.startswith("+ "):
            only_b.append(ln[2:])
    return only_a, only_b


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_lazy_lim_changes_only_the_limit(bodies, dt):
    on = _functions(bodies["default"][1])[f"fwdpp_plain_item_{dt}"]
    off = _functions(bodies["nolazy"][1])[f"fwdpp_plain_item_{dt}"]
    only_off, only_on = _changed(off, on)
    assert set(only_off) == {"v_add_u32 v59, -64, v59"}
    assert set(only_on) == {"s_mov_b32 s88, -1", "s_add_i32 s89, s88, 1", "s_lshl_b32 s89, s89, 6",
                            "v_subrev_u32 v59, s89, %[lim]"}
    # per group: one step per V phase (1 pre-loop + 1 no-key + 4 ring phases x (unmasked, masked,
    # last, idle)) against one formation per masked V phase (pre-loop + 4) and the rare path
    assert len(only_off) == 2 * 18 and only_on.count("v_subrev_u32 v59, s89, %[lim]") == 2 * 6


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_max0_changes_only_the_first_max(bodies, dt):
    on = _functions(bodies["default"][1])[f"fwdpp_plain_item_{dt}"]
    off = _functions(bodies["nomax0"][1])[f"fwdpp_plain_item_{dt}"]
    only_off, only_on = _changed(off, on)
    assert only_off == []
    want = []
    for g in "AB":
        want += ["s_cmp_gt_i32 %[ew], 0", f"s_cbranch_scc0 .Lfmm_{g}_%="]
        want += [f"v_max_f32 v60, v60, v{v}" for v in range(32)]
        want += [f"s_branch .Lfmj_{g}_%=", f".Lfmm_{g}_%=:", f".Lfmj_{g}_%=:"]
    assert only_on == want
