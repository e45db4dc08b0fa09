"""Generate csrc/fmha_fwd8pp_body.h: the 8-wave ping-pong fp8 (e4m3fn) forward body
(csrc/fmha_fwd8pp_kernel.h).

The phase program of tools/gen_fwdpp.py (read its docstring: two waves per SIMD, waves 4-7 one
phase behind waves 0-3, MFMA phases PV(j) + QK^T(j+1) against VALU phases softmax(j+1) +
LDS-DMA, the unmasked / masked / last / idle step variants, the rare redo path) on the operand
layouts of the 4-wave fp8 kernel (tools/gen_fwd8.py): both GEMMs on the block-scaled
v_mfma_scale_f32_32x32x64_f8f6f4 (E8M0 scales 1.0, 64 cycles per MFMA), a wave of 32 query rows
per 64-key tile runs 4 QK^T + 4 PV MFMAs (512 cycles) against its 32 scores' softmax, which is
where the 4-wave fp8 kernel spent its time (VALU-bound): here the partner wave's
MFMAs run beside it.

The body is a subclass of gen_fwdpp.PingPong: it states its own register map, options and
parameters (wait states, DMA pieces, the v_scale epilogue factor) and overrides the
operand-specific methods (fragment reads, MFMAs, P packing, DMA pieces, Q loads), so the phase
logic and the read scheduler exist once.

Register map (per lane, 256 = v[0:127] + a[0:127]):
  a[0:63]    O^T accumulators (4 d tiles x 16)
  a[64:79]   Q fragments (2 x 8: d 0-63, 64-127; 32 bytes per lane each)
  a[80:111]  K fragment ring (4 slots x 8: one tile's (kt, s) fragments)
  v[0:31]    S;  v[32:39] P (8 dwords of e4m3, the B operand of PV with the k permutation of
             gen_fwd8.py);  v[40:47] scratch;  v48 tile row sum, v49 -m, v50 running sum,
  v51 key limit, v52-55 redo / max temps, v56 = 127 (E8M0 scale 1.0)
  v[64:95]   V^T fragment ring (4 slots x 8)

  python tools/gen_fwd8pp.py       (writes xf_flash_attention_cutlass_amd/csrc/fmha_fwd8pp_body.h)
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import asmgen  # noqa: E402
from gen_fwdpp import PingPong, place_reads, spans  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "xf_flash_attention_cutlass_amd", "csrc", "fmha_fwd8pp_body.h")

MNEM = "v_mfma_scale_f32_32x32x64_f8f6f4"


class PingPongFp8(PingPong):
    """The fp8 body (fwd8pp_item_* by output dtype); options: abl."""
    NAME = "fwd8pp"
    TILE = 64 * 128        # one fp8 K (or V) tile
    LEAD = 4               # gaps a K fragment read leads its MFMA
    # register map
    SBASE, PBASE, TMP = 0, 32, 40
    LT, NM, LRUN, LIM, MISC = 48, 49, 50, 51, 52
    SC127 = 56
    ABASE_O, ABASE_Q, ABASE_K, VBASE_V = 0, 64, 80, 64
    SKR, SVR = 80, 84
    SJ, ST, SST, SRA, SCM = 88, 89, 90, 92, 94
    # options
    FEATURES = False       # (no softcap / ALiBi pass in this body)
    LEFTWIN = False        # (no left windows: the one-sided key limit)
    DMAMIX = True
    # parameters (gen_fwdpp.PingPong explains them)
    RING, DLEAD = 4, 3
    NPIECE = 2             # one K and one V piece per wave and tile (8 KiB tiles, 8 waves)
    EPI_SCALE = "%[vsc]"
    # the 32x32x64 fp8 MFMA's results: 40 wait states before a VALU reads them (gen_fwd8.py)
    XDL_NOPS = ["s_nop 7"] * 5
    VPH_NOPS = ["s_nop 7"] * 5
    N_EPI_STORES = 9       # 8 O row stores + the LSE store

    SIG = ("const int kblo, const int kbhi, const int vblo, const int vbhi, const int kvbytes, "
           "const i32x4 qsrd, const i32x4 osrd, const i32x4 lsrd, const int kstep, const int kdst, "
           "const int ntl, const int tw, const int ew, const int grp, const float c, const float thr, "
           "const float vsc, const int ka0, const int ka1, const int ka2, const int ka3, const int va0, "
           "const int va1, const int va2, const int va3, const int dk, const int dv, const int lim, "
           "const int qoff, const int ooff, const int loff")
    INS = (asmgen.operands("s", "kblo kbhi vblo vbhi kvbytes qsrd osrd lsrd kstep kdst ntl tw ew grp c thr vsc") +
           asmgen.operands("v", "ka0 ka1 ka2 ka3 va0 va1 va2 va3 dk dv lim qoff ooff loff"))

    def qtup(self, s):
        return f"a[{self.ABASE_Q + 8 * s}:{self.ABASE_Q + 8 * s + 7}]"

    def ktup(self, slot, half=None):
        b = self.ABASE_K + 8 * slot
        return f"a[{b}:{b + 7}]" if half is None else f"a[{b + 4 * half}:{b + 4 * half + 3}]"

    def vtup(self, slot, kb=None):
        b = self.VBASE_V + 8 * slot
        return f"v[{b}:{b + 7}]" if kb is None else f"v[{b + 2 * kb}:{b + 2 * kb + 1}]"

    def value_info(self, v):
        """score v (kt*16 + r): key offset in the tile minus 4*hh, P dword (4 e4m3 per dword)"""
        kt, r = v // 16, v % 16
        return 32 * kt + 8 * (r >> 2) + (r & 3), 4 * kt + (r >> 2)

    def cvt_pair(self, dt, v, dword, lo, hi):
        """P = e4m3(exp2(S c - m)): scores v - 1, v into a half of P dword `dword` (gen_fwd8.py's
        ops; the rest of PingPong.softmax stands: fp32 row sum in LT)"""
        sel = " op_sel:[0,0,1]" if (v % 16) & 3 == 3 else ""
        return f"v_cvt_pk_fp8_f32 v{self.PBASE + dword}, {lo}, {hi}{sel}"

    def k_reads(self, f, slot_tile):
        kt, s = f // 2, f % 2
        return [f"ds_read_b128 {self.ktup(f, u)}, %[ka{2 * s + u}] offset:{slot_tile * self.TILE + kt * 32 * 128}"
                for u in (0, 1)]

    def v_reads(self, dt_, slot_tile):
        return [f"ds_read_b64_tr_b8 {self.vtup(dt_, kb)}, %[va{dt_}] offset:{slot_tile * self.TILE + kb * 2048}"
                for kb in range(4)]

    def m_phase(self, dt, j_slot, pv=True, qk=True):
        """PV(j) (4 MFMAs) then QK^T(j+1) (4 MFMAs); with qk, tile j+1's 4 V^T fragments are read at
        the end (the next PV's operands).  On entry with pv, this tile's V^T fragments (16 reads)
        are the only LDS reads in flight."""
        sc = f"v{self.SC127}, v{self.SC127} op_sel_hi:[0,0,0]"
        nx = (j_slot + 1) % self.RING
        mf = []
        if pv:
            for d in range(4):
                mf.append((("V", d), f"{MNEM} {self.otup(d)}, {self.vtup(d)}, "
                                     f"v[{self.PBASE}:{self.PBASE + 7}], {self.otup(d)}, {sc}"))
        if qk:
            for f in range(4):
                kt, s = f // 2, f % 2
                acc = self.sv(kt)
                mf.append((("K", f), f"{MNEM} {acc}, {self.ktup(f)}, {self.qtup(s)}, {acc if s else '0'}, {sc}"))
        G = len(mf)
        first, last = spans(mf)
        reads = []
        if qk:
            for f in range(4):
                g = max(first[("K", f)] - self.LEAD, 0) if first[("K", f)] > 0 else -1
                reads.append((g, 0, self.k_reads(f, nx), ("K", f)))
            for d in range(4):
                lo = (last[("V", d)] + 2) if pv else 0
                g = max(lo, G - 8 + 2 * d)
                reads.append((min(g, G), 2 + d, self.v_reads(d, nx), ("N", d)))
        return place_reads(mf, reads, [(("V", d), 4) for d in range(4)] if pv else [])

    def dma_pieces(self, slot):
        """this wave's K piece and V piece of the tile in slot (8 rows x 128 bytes each)"""
        out = []
        for op, srd, base in (("dk", self.SKR, 0), ("dv", self.SVR, self.RING * self.TILE)):
            out.append([f"s_add_u32 m0, %[kdst], {base + slot * self.TILE}", "s_nop 0",
                        f"buffer_load_dwordx4 %[{op}], s[{srd}:{srd + 3}], 0 offen lds"])
        return out

    def item_program(self, dt):
        out = ["s_waitcnt lgkmcnt(0)",
               f"v_mov_b32 v{self.NM}, 0", f"v_mov_b32 v{self.LRUN}, 0", f"v_mov_b32 v{self.LIM}, %[lim]",
               f"v_mov_b32 v{self.SC127}, 0x7f", f"s_mov_b32 s{self.SST}, 0"]
        # Q fragments: s -> 2 x 16 bytes at d = 64 s + 32 hh (+ 16)
        for s in range(2):
            for u in range(2):
                b = self.ABASE_Q + 8 * s + 4 * u
                out.append(f"buffer_load_dwordx4 a[{b}:{b + 3}], %[qoff], %[qsrd], 0 offen offset:{64 * s + 16 * u}")
        out += [f"v_accvgpr_write_b32 a{self.ABASE_O + i}, 0" for i in range(64)]
        out += self.dense_descriptors()
        for slot in range(self.DLEAD - 1):                       # tiles 0 .. DLEAD-2
            out += sum(self.dma_pieces(slot), []) + self.dma_advance()
        # Q and tile 0 landed, published
        out += [f"s_waitcnt vmcnt({self.NPIECE * (self.DLEAD - 2)})", "s_barrier"]
        return out + self.groups(dt)


def emit(out=OUT, **options):
    """options: abl"""
    body = PingPongFp8(**options)
    asmgen.write_header(
        out, "gen_fwd8pp.py",
        ["// The 8-wave ping-pong fp8 forward's item body (fmha_fwd8pp_kernel.h): one asm statement",
         "// per output dtype with a fixed register map; see the generators' docstrings."],
        [ln for dt in ("bf16", "f16") for ln in body.function(dt)],
        decls=[f"constexpr int kFwd8ppRing = {body.RING};          // K / V tile slots the body addresses"])


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--abl", default="", help="timing ablations, comma list (results invalid)")
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    emit(a.out, abl=[x for x in a.abl.split(",") if x])
