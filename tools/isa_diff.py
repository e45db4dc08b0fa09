"""Is the device code of two source trees the same?  Compiles every translation unit build.py
compiles (and the ones XFA_VARIANTS=1 rebuilds) device-only to assembly with build.py's flags,
in both trees, and compares kernel by kernel after renumbering the .LBB labels and dropping the
assembler comments (which name labels by the function's index in its unit).  Only the
__hip_cuid_<hash> symbol (a hash of the source text) may differ.  A kernel only one tree has is
listed as ONLY IN A / B and does not count as a difference.

  python tools/isa_diff.py <tree A> <tree B> [-j N] [--kernarg] [--rename REGEX=REPL]
                                                          exit status 1 if any kernel differs

--kernarg: for trees whose parameter blocks differ in size (a field added at the end): the
kernarg size and the offsets of scalar loads / address adds from the kernarg pointer s[0:1] are
masked, so a kernel counts as identical when nothing but where its arguments lie has changed.
--rename REGEX=REPL: applied to tree A's assembly first, for a kernel template that gained a
parameter in tree B (its instantiations' mangled names then differ though their code may not), e.g.
  --rename 'fmha_fwdpp_kernelILb(\d)ELb(\d)ELb(\d)EEE=fmha_fwdpp_kernelILb\1ELb\2ELb\3ELb0EEE'
The labels of inline asm statements (.L<name>_<n>, n = the statement's %= number, which counts the
asm statements the compiler has seen before it) are renumbered per kernel like the .LBB ones.
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
    if hasattr(b, "generate"):
        b.generate()               # (the headers the build generates before compiling)
    tus = [(f"fmha_{kind}_hd{hd}_{dt}", f"fmha_{kind}.hip",
            [f"-DXFA_HD={hd}", f"-DXFA_DTN={dt}", f"-DXFA_DT_BF16={int(dt == 'bf16')}"])
           for hd, dt in b.VARIANTS for kind in ("fwd", "bwd")]
    tus += [("fmha_append", "fmha_append.hip", []), ("fmha_quant", "fmha_quant.hip", []),
            ("fmha_fwd_fp8", "fmha_fwd_fp8.hip", []), ("fmha_api", "fmha_api.cpp", []),
            ("fmha_merge", "fmha_merge.hip", []),
            ("fmha_mla", "fmha_mla.hip", ["-mllvm", "-amdgpu-mfma-vgpr-form"])]   # (build.py's flag)
    if os.path.exists(os.path.join(b.CSRC, "fmha_fwd_mla.hip")):      # (trees from 2.12 on)
        tus += [(f"fmha_fwd_mla_{dt}", "fmha_fwd_mla.hip", [f"-DXFA_DTN={dt}", f"-DXFA_DT_BF16={int(dt == 'bf16')}"])
                for dt in ("bf16", "f16")]
    if os.path.exists(os.path.join(b.CSRC, "fmha_bwd_mla.hip")):      # (trees from 2.13 on)
        tus += [(f"fmha_bwd_mla_{dt}", "fmha_bwd_mla.hip", [f"-DXFA_DTN={dt}", f"-DXFA_DT_BF16={int(dt == 'bf16')}"])
                for dt in ("bf16", "f16")]
    tus += [(n + "+variants", src, d + ["-DXFA_VARIANTS=1"]) for n, src, d in tus if n + ".o" in b.VARIANT_TUS]
    return b, tus


MASK_KERNARG = False
RENAME = None       # (regex, replacement) for tree A's assembly


def kernels(tree, tu, out_dir):
    """{kernel symbol: normalised body} of one translation unit"""
    b, (name, src, defs) = tu
    asm = os.path.join(out_dir, name + ".s")
    subprocess.run([b.HIPCC, "-x", "hip", *b.HIP_FLAGS, *defs, "--cuda-device-only", "-S",
                    os.path.join(b.CSRC, src), "-o", asm], check=True)
    text = open(asm).read()
    if RENAME and tree == RENAME[2]:
        text = re.sub(RENAME[0], RENAME[1], text)
    return name, normalise(text)


def normalise(text):
    """{kernel symbol: normalised body + kernel descriptor} of one unit's assembly"""
    text = re.sub(r"(?m)^.*__hip_cuid_.*\n", "", text)
    if MASK_KERNARG:
        text = re.sub(r"\.amdhsa_kernarg_size \d+", ".amdhsa_kernarg_size <n>", text)
        text = re.sub(r"(?m)^(\s*s_load_dword\w* \S+ s\[0:1\], |\s*s_add_u32 s\d+, s0, |\s*s_addc_u32 s\d+, s1, )0x[0-9a-f]+",
                      r"\1<kernarg>", text)
    out = {}
    for m in re.finditer(r"(?ms)^(\w+):.*?^\.Lfunc_end\d+:", text):
        labels = {}
        body = re.sub(r"\.Lfunc_end\d+", ".Lfunc_end", m.group(0))     # (a function's index in its unit)
        body = re.sub(r"(?m)[ \t]*;.*$", "", body)
        body = re.sub(r"\.LBB\d+_\d+", lambda l: labels.setdefault(l.group(0), f".L{len(labels)}"), body)
        far = {}    # the compiler's long-branch labels, numbered through the unit
        body = re.sub(r"\.Lpost_getpc\d+", lambda l: far.setdefault(l.group(0), f".Lpost_getpc<{len(far)}>"), body)
        ids = {}    # inline asm labels: the %= number of their statement
        out[m.group(1)] = re.sub(r"(\.L[A-Za-z][A-Za-z0-9_]*_)(\d+)\b",
                                 lambda l: l.group(1) + ids.setdefault(l.group(2), f"<{len(ids)}>"), body)
    for m in re.finditer(r"(?ms)^\s*\.amdhsa_kernel (\w+)\n.*?\.end_amdhsa_kernel", text):
        out[m.group(1)] += m.group(0)          # registers, LDS, the kernel descriptor's settings
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("trees", nargs=2)
    ap.add_argument("-j", type=int, default=8)
    ap.add_argument("--kernarg", action="store_true", help="mask kernarg size and offsets")
    ap.add_argument("--rename", default="", help="REGEX=REPL applied to tree A's assembly")
    a = ap.parse_args()
    global MASK_KERNARG, RENAME
    MASK_KERNARG = a.kernarg
    if a.rename:
        RENAME = (*a.rename.split("=", 1), a.trees[0])
    res, bad = [], 0
    with tempfile.TemporaryDirectory() as tmp, cf.ThreadPoolExecutor(a.j) as ex:
        for i, tree in enumerate(a.trees):
            b, tus = units(tree)
            os.makedirs(os.path.join(tmp, str(i)))
            res.append(dict(ex.map(lambda tu: kernels(tree, (b, tu), os.path.join(tmp, str(i))), tus)))
    for name in sorted(set(res[0]) | set(res[1])):
        ka, kb = res[0].get(name, {}), res[1].get(name, {})
        diff = sorted(k for k in set(ka) & set(kb) if ka[k] != kb[k])
        bad += len(diff)
        print(f"{name}: {len(ka)} kernels, {len(set(ka) & set(kb)) - len(diff)} identical"
              + "".join(f"\n  DIFFERS {k}" for k in diff)
              + "".join(f"\n  ONLY IN A {k}" for k in sorted(set(ka) - set(kb)))
              + "".join(f"\n  ONLY IN B {k}" for k in sorted(set(kb) - set(ka))))
    print("device code identical" if not bad else f"{bad} kernels differ")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
