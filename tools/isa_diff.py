"""Is the device code of two source trees the same?  Compiles every translation unit build.py
compiles (and the ones XFA_VARIANTS=1 rebuilds) device-only to assembly with build.py's flags,
in both trees, and compares kernel by kernel after renumbering the .LBB labels.  Only the
__hip_cuid_<hash> symbol (a hash of the source text) may differ.

  python tools/isa_diff.py <tree A> <tree B> [-j N]      exit status 1 if any kernel differs
"""
import argparse
import concurrent.futures as cf
import importlib.util
import os
import re
import subprocess
import sys
import tempfile


def units(tree):
    spec = importlib.util.spec_from_file_location("b", os.path.join(tree, "xf_flash_attention_cutlass_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    tus = [(f"fmha_{kind}_hd{hd}_{dt}", f"fmha_{kind}.hip",
            [f"-DXFA_HD={hd}", f"-DXFA_DTN={dt}", f"-DXFA_DT_BF16={int(dt == 'bf16')}"])
           for hd, dt in b.VARIANTS for kind in ("fwd", "bwd")]
    tus += [("fmha_append", "fmha_append.hip", []), ("fmha_quant", "fmha_quant.hip", []),
            ("fmha_fwd_fp8", "fmha_fwd_fp8.hip", []), ("fmha_api", "fmha_api.cpp", [])]
    tus += [(n + "+variants", src, d + ["-DXFA_VARIANTS=1"]) for n, src, d in tus if n + ".o" in b.VARIANT_TUS]
    return b, tus


def kernels(tree, tu, out_dir):
    """{kernel symbol: normalised body} of one translation unit"""
    b, (name, src, defs) = tu
    asm = os.path.join(out_dir, name + ".s")
    subprocess.run([b.HIPCC, "-x", "hip", *b.HIP_FLAGS, *defs, "--cuda-device-only", "-S",
                    os.path.join(b.CSRC, src), "-o", asm], check=True)
    text = re.sub(r"(?m)^.*__hip_cuid_.*\n", "", open(asm).read())
    out = {}
    for m in re.finditer(r"(?ms)^(\w+):.*?^\.Lfunc_end\d+:", text):
        labels = {}
        out[m.group(1)] = re.sub(r"\.LBB\d+_\d+", lambda l: labels.setdefault(l.group(0), f".L{len(labels)}"), m.group(0))
    for m in re.finditer(r"(?ms)^\s*\.amdhsa_kernel (\w+)\n.*?\.end_amdhsa_kernel", text):
        out[m.group(1)] += m.group(0)          # registers, LDS, the kernel descriptor's settings
    return name, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("trees", nargs=2)
    ap.add_argument("-j", type=int, default=8)
    a = ap.parse_args()
    res, bad = [], 0
    with tempfile.TemporaryDirectory() as tmp, cf.ThreadPoolExecutor(a.j) as ex:
        for i, tree in enumerate(a.trees):
            b, tus = units(tree)
            os.makedirs(os.path.join(tmp, str(i)))
            res.append(dict(ex.map(lambda tu: kernels(tree, (b, tu), os.path.join(tmp, str(i))), tus)))
    for name in sorted(set(res[0]) | set(res[1])):
        ka, kb = res[0].get(name, {}), res[1].get(name, {})
        diff = sorted(k for k in set(ka) | set(kb) if ka.get(k) != kb.get(k))
        bad += len(diff)
        print(f"{name}: {len(ka)} kernels, {len(ka) - len([k for k in diff if k in ka])} identical"
              + "".join(f"\n  DIFFERS {k}" for k in diff))
    print("device code identical" if not bad else f"{bad} kernels differ")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
