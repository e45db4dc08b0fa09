"""CPU checks of tests/decode_util.py: the evidence that the shapes of
tests/test_decode_instances_gpu.py are sharp enough.

* The clean CPU model of a split decode passes the GPU file's pass rule against the oracle on every
  shape family and with every fill, and every planted defect fails it.  What a family cannot
  catch: `combine_ns` needs dec_bal (the "bal" mappings catch it), `no_v_scale` needs an fp8 cache
  (every fp8 family catches it), `second_page` needs more than one page (every paged family
  catches it; the one-page leftpad families cannot), `k_tail` needs a right window that reaches
  past the last key (causal and (64, 0) hide it; every other family catches it).
* The chosen lengths hit the kernel's loop structure (checked with the Python port of its split
  arithmetic): for every ring depth the splits own r and RING + r tiles for every r < RING, some
  split owns none, every tile straddles a page edge, the dec_bal shares are unequal and one is 1.
  A share limited by dec_cap needs more than 128 slots, i.e. more than the 5 sequences x 16 splits
  a 1024-key table allows: LENS_CAP over a 2048-key table is the one shape that leaves that limit.
* The dec_slot shares of the port: they sum to dec_slots, each is at least 1, equal lengths give
  num_splits.
"""
import pytest
import torch

from tests import decode_util as du

FAMILIES = [du.Instance(64, torch.float16 if i % 2 else torch.bfloat16, fp8, mr, m)
            for i, (fp8, mr, m) in enumerate((f, r, m) for f in (False, True) for r in (16, 32)
                                             for m in du.MAPPINGS)]


def _emu(c, q, plan, defect=None):
    return du.emulate_decode(c, q, plan["splits"], plan["bal"], plan["slots"], plan["cap"],
                             defect=defect)


def _catchable(defect, c, plan):
    if defect == "combine_ns":
        return plan["bal"]
    if defect == "no_v_scale":
        return c.fp8
    if defect == "second_page":
        return c.width > 1
    return True


def _check_family(problem):
    c, q, plan = problem("nan")
    ora = du.oracle(c, q)
    for fill in du.FILLS:
        cf = c if fill == "nan" else problem(fill)[0]
        o, lse = _emu(cf, q, plan)
        ok, f = du.judge(o, lse, ora)
        assert ok, f"clean model, fill {fill}: {f}"
    for defect in du.DEFECTS:
        if not _catchable(defect, c, plan):
            continue
        o, lse = _emu(c, q, plan, defect)
        ok, f = du.judge(o, lse, ora)
        assert not ok, f"defect {defect} passes the rule: {f}"
    # the tail defects need a non-finite tail: over zeros the V tail is invisible
    cz = problem("zero")[0]
    assert du.judge(*_emu(cz, q, plan, "v_tail"), ora)[0]
    assert not du.judge(*_emu(cz, q, plan, "k_tail"), ora)[0]


@pytest.mark.parametrize("t", FAMILIES, ids=du.instance_name)
def test_model_instance_family(t):
    _check_family(lambda fill: du.instance_problem(t, fill))


@pytest.mark.parametrize("fc", du.FILL_CASES, ids=du.fill_name)
def test_model_fill_family(fc):
    _check_family(lambda fill: du.fill_problem(fc, fill))


def _check_feature(c, q, plan, kw, mult):
    ora = du.oracle(c, q, **kw)
    emu = lambda defect=None: du.emulate_decode(c, q, plan["splits"], plan["bal"], plan["slots"],  # noqa: E731
                                                plan["cap"], defect=defect, **kw)
    ok, f = du.judge(*emu(), ora, mult)
    assert ok, f"clean model: {f}"
    for defect in ("v_tail", "k_tail", "drop_last_tile", "second_page", "combine_ns"):
        if defect == "k_tail" and kw["window"][1] == 0:
            continue        # a right window of 0 ends at the last key: it hides a lost end
        ok, f = du.judge(*emu(defect), ora, mult)
        assert not ok, f"defect {defect} passes the rule: {f}"


@pytest.mark.parametrize("sq", [1, 4])
@pytest.mark.parametrize("window", list(du.WINDOWS))
def test_model_window_family(window, sq):
    c, q, plan = du.window_problem(sq)
    assert plan["bal"]
    _check_feature(c, q, plan, dict(window=du.WINDOWS[window]), 3.0)


@pytest.mark.parametrize("name", list(du.FEATURES))
def test_model_feature_family(name):
    c, q, plan, kw, mult = du.feature_problem(name)
    assert plan["bal"]
    _check_feature(c, q, plan, kw, mult)


def test_instance_table_complete():
    tab = du.instance_table()
    assert len(tab) == len(set(tab)) == 16 * 5
    # the 32 template instances: (head size, dtype, cache, rows) x (4 | 8 waves)
    assert len({(t.d, t.dtype, t.fp8, t.mr, t.mapping in ("hmaj2", "bal2")) for t in tab}) == 32
    assert {t.mapping for t in tab} == set(du.MAPPINGS)
    assert len({du.instance_name(t) for t in tab}) == len(tab)


def _owned(mapping, mr):
    hk, group, sq, lens, knobs = du.mapping_shape(mapping, mr)
    splits, hm, bal, slots, cap = du.host_plan(len(lens), hk, du.WIDTH * du.PAGE, du.NUM_SPLITS,
                                               knobs["dec_hmaj"], knobs["dec_bal"])
    assert splits == du.NUM_SPLITS and hm == knobs["dec_hmaj"] and bal == bool(knobs["dec_bal"])
    return du.split_tiles(lens, sq, group, (-1, -1), du.WIDTH * du.PAGE, splits, bal, slots, cap), cap


@pytest.mark.parametrize("mapping", du.MAPPINGS)
@pytest.mark.parametrize("fp8,mr", [(False, 16), (False, 32), (True, 32), (True, 16)])
def test_lengths_hit_the_loop_structure(mapping, fp8, mr):
    ring = du.ring_depth(fp8, mr)
    assert ring == {(False, 16): 1, (False, 32): 1, (True, 32): 2, (True, 16): 3}[(fp8, mr)]
    st, cap = _owned(mapping, mr)
    counts = {n for _, own in st for n in own}
    for r in range(ring):
        assert r in counts and ring + r in counts, (ring, r, st)
    assert 0 in counts
    assert du.TILE > du.PAGE and du.TILE % du.PAGE == 0      # every tile holds a page edge
    if mapping.startswith("bal"):
        shares = [nb for nb, _ in st]
        assert len(set(shares)) > 1 and 1 in shares, shares
        assert sum(shares) == 5 * du.NUM_SPLITS and max(shares) < cap


def test_lengths_cover_the_edges():
    lens = set(du.LENS_UNIFORM) | set(du.LENS_BAL) | set(du.LENS_EDGE)
    eff = {n - p for n, p in zip(du.ONEPAGE_LENS, du.ONEPAGE_LEFTPAD)}
    assert {1024, 32, 1, 0} <= lens and 0 in eff and 32 in eff
    assert any(n % 32 and n % du.PAGE for n in lens)
    assert max(lens) <= 1024 and du.ONEPAGE % 16 == 0 and max(du.ONEPAGE_LENS) <= du.ONEPAGE
    assert all(p % 8 for p in du.ONEPAGE_LEFTPAD)


def test_dec_cap_needs_the_larger_table():
    # within the module's limits (5 sequences, 1024 keys -> at most 16 splits) the cap is the slot
    # count itself and no share can reach it
    splits, _, bal, slots, cap = du.host_plan(5, 4, 1024, 128, 1, 1)
    assert (splits, bal, slots, cap) == (16, True, 80, 80)
    # the cap case: 2048 keys -> 32 splits, 160 slots, cap 128
    splits, _, bal, slots, cap = du.host_plan(len(du.LENS_CAP), 4, du.CAP_WIDTH * du.PAGE, 32, 1, 1)
    assert (splits, slots, cap) == (32, 160, 128)
    tiles = [(n + du.TILE - 1) // du.TILE for n in du.LENS_CAP]
    raw = du.bal_shares(tiles, slots, 10 ** 9)
    got = du.bal_shares(tiles, slots, cap)
    assert max(raw) > cap and max(got) == cap and sum(got) < slots


def test_bal_shares_properties():
    gen = torch.Generator().manual_seed(3)
    for _ in range(300):
        b = int(torch.randint(2, 65, (1,), generator=gen))
        splits = 4 * int(torch.randint(1, 33, (1,), generator=gen))
        tiles = [int(x) for x in torch.randint(0, 1025, (b,), generator=gen)]
        slots = b * splits
        n = du.bal_shares(tiles, slots, 10 ** 9)
        assert min(n) >= 1 and sum(n) == (slots if sum(tiles) else b)
        capped = du.bal_shares(tiles, slots, min(slots, 128))
        assert all(1 <= x <= min(slots, 128) for x in capped) and sum(capped) <= slots
        assert du.bal_shares([tiles[0]] * b, slots, 128) == [min(splits, 128) if tiles[0] else 1] * b
