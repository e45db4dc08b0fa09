"""bench.py's plain run, --full switch and --dump-outputs.

CPU: the option parsing and sample_outputs (what --dump-outputs keeps of a step's outputs: whole
arrays within the byte budget, else the same seeded sample of each in every run).  GPU: one tiny
plain run with --dump-outputs through the HIP forward (a run of the benchmark itself, because
the option is what the test is about); the shape is small enough to be dumped whole, and the
dumped output is checked against the CPU oracle on the regenerated inputs.
"""
import json
import os
import subprocess
import sys

import pytest
import torch

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_is_the_default():
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert not a.full and a.dump_outputs is None and a.steps == 7 and a.warmup == 2
    a = bench.parse(["--full", "--dump-outputs", "d"])
    assert a.full and a.dump_outputs == "d"
    with pytest.raises(SystemExit):
        bench.parse(["--steps", "0"])


def test_sample_outputs_whole_when_small():
    outs = {"out": torch.arange(24, dtype=torch.bfloat16).view(2, 3, 4),
            "softmax_lse": torch.tensor([[0.5, float("-inf")]])}
    got = bench.sample_outputs(outs)
    assert list(got) == ["out", "softmax_lse"]
    for n, t in outs.items():
        assert got[n].dtype == torch.float32 and got[n].shape == t.shape
        assert torch.equal(got[n], t.float())


def test_sample_outputs_fixed_sample_within_budget(monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BYTES", 4 * 1000)
    g = torch.Generator().manual_seed(3)
    outs = {"big": torch.randn(50, 97, generator=g), "small": torch.randn(11, generator=g),
            "big2": torch.randn(4001, generator=g).double()}
    a, b = bench.sample_outputs(outs), bench.sample_outputs(outs)
    assert sum(t.numel() * t.element_size() for t in a.values()) <= 4 * 1000
    assert a["small"].shape == (11,) and torch.equal(a["small"], outs["small"])
    for n in ("big", "big2"):
        assert a[n].dtype == torch.float32 and a[n].shape == (1000 // 3,)
        assert torch.equal(a[n], b[n])                    # the same elements run to run
        # the sample is a gather of the flattened array at increasing, distinct indices
        src = outs[n].reshape(-1).float()
        it = iter(src.tolist())
        assert all(any(x == y for y in it) for x in a[n].tolist())


@pytest.mark.gpu
def test_plain_run_dumps_the_last_steps_outputs(tmp_path):
    import numpy as np
    from oracle import attention_ref as orc
    B, S, H, D = 2, 192, 4, 128
    args = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--prewarm-s", "0", "--batch", str(B),
            "--seqlen", str(S), "--heads", str(H), "--dump-outputs", str(tmp_path)]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args],
                       capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["ms_per_step"] > 0 and d["unit"] == "TFLOP/s"
    assert d["dtype"] == "bf16" and d["higher_is_better"] is True
    # a plain run measures nothing but its headline figure
    for k in ("roofline", "cpu_baseline", "gpu_clock", "fwd_bwd", "varlen", "decode", "fwd_fp8"):
        assert k not in d, k
    assert sorted(os.listdir(tmp_path)) == ["out.npy", "softmax_lse.npy"]
    out = np.load(tmp_path / "out.npy")
    lse = np.load(tmp_path / "softmax_lse.npy")
    assert out.dtype == np.float32 and out.shape == (B, S, H, D)
    assert lse.dtype == np.float32 and lse.shape == (B, H, S)
    # no prewarm, 1 warmup and 3 timed steps over 2 rotating input sets: the last step read set
    # 1, the second (q, k, v) draw of bench.py's device generator (seed 1234 + rank)
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(1234)
    for _ in range(2):
        q, k, v = (torch.randn(B, S, H, D, device=dev, dtype=torch.bfloat16, generator=g).cpu()
                   for _ in range(3))
    ref, _ = orc.attention_ref(q, k, v, causal=True)
    pt, _ = orc.attention_ref(q, k, v, causal=True, upcast=False, reorder_ops=True)
    ok, err, bound = orc.parity_ok(torch.from_numpy(out).bfloat16(), ref, pt, 2.0)
    assert ok, f"dumped out differs from the oracle: {err} > {bound}"
