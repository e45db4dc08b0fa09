"""Generate csrc/fmha_fwdpp16_body.h: the 8-wave ping-pong D = 128 forward body on the bf16 /
f16 MFMA shape v_mfma_f32_16x16x32 (csrc/fmha_fwdpp_kernel.h with M16).

The phase program of tools/gen_fwdpp.py (read its docstring: two waves per SIMD, waves 4-7 one
phase behind waves 0-3, MFMA phases PV(j) + QK^T(j+1) against VALU phases softmax(j+1) +
LDS-DMA, the unmasked / masked / last / idle step variants, the rare redo path) with the same
output tile per wave (32 query rows x 64 keys per step) on the 16x16x32 shape.  Why: at the
1.4 kW board cap the chip holds a higher clock on 16x16x32 than on 32x32x16 at equal cycles per
FLOP (MI355X_MICROARCH.md DVFS give-back item 7; probe tools/gen_pingpong16.py: +5 % per
second on the full ping-pong, +6 % clock).  Like gen_fwd8pp.py's, this body is a subclass of
gen_fwdpp.PingPong: it states its own register map and options and overrides the
operand-specific methods, so the phase logic and the read scheduler exist once.

Layout per wave (its 32 query rows = two 16-row tiles rt; g = lane >> 4, l16 = lane & 15):
  S^T(kt, rt) = K(kt) Q^T(rt)   16 keys x 16 rows over 4 k-steps of 32 d; a lane holds row
                                16 rt + l16 and keys 16 kt + 4 g + r (r = 0..3)   32 MFMAs
  O^T(dt, rt) += V^T(dt) P^T    16 d x 16 rows over 2 k-steps of 32 keys; k index m of lane
                                group g = key 32 ks + 16 (m >> 2) + 4 g + (m & 3): P(ks, rt) is
                                cvt_pk of S^T(2 ks, rt), S^T(2 ks + 1, rt) as they stand, the
                                V^T fragment two ds_read_b64_tr_b16 blocks 16 keys apart  32 MFMAs
  K fragment (kt, s): ds_read_b128 at kv_off(16 kt + l16, 4 s + g) (one base register)
  a row's 64 keys of a tile sit on the 4 lanes l16 + 16 g: row max / row sum reductions take a
  permlane32 and a permlane16 swap; each lane carries two rows (limit, -m, sums per row)

Register map (per lane, 256 = v[0:127] + a[0:127]):
  a[0:63]    O^T (8 dt x 2 rt x 4)         a[64:95]  Q (2 rt x 4 s x 4)
  a[96:127]  K fragment ring (8 x 4)
  v[0:31]    S (v = 8 kt + 4 rt + r)       v[32:47]  P (2 ks x 2 rt x 4 packed pairs)
  v[48:55]   softmax scratch               v[64:95]  V^T fragment ring (8 x 4)
  v56/57 tile row sums (rt 0 / 1), v58/59 -m, v60/61 running row sums, v62/63 key limits
  v[96:103]  max / redo temps

  python tools/gen_fwdpp16.py      (writes xf_flash_attention_cutlass_amd/csrc/fmha_fwdpp16_body.h)
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import asmgen  # noqa: E402
from gen_fwdpp import PingPong  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "xf_flash_attention_cutlass_amd", "csrc", "fmha_fwdpp16_body.h")


class PingPong16(PingPong):
    """The 16x16x32 bf16 / f16 body (fwdpp16_item_*); options: stamps, lead."""
    NAME = "fwdpp16"
    KS, VS = 8, 8          # fragment ring slots
    LEAD = 6               # MFMA gaps (16x16x32: half the 32x32x16 cycles) an LDS read leads its MFMA
    NVPRE = 4              # V^T fragments of the next PV read at the end of an M phase
    TAIL_GAP = 4           # MFMA gaps between those reads (two fragments' worth)
    # register map
    SBASE, PBASE, TMP = 0, 32, 48
    LT, NM, LRUN, LIM, MISC = 56, 58, 60, 62, 96      # pairs: register + rt
    ABASE_O, ABASE_Q, ABASE_K, VBASE_V = 0, 64, 96, 64
    SKR, SVR = 80, 84
    SJ, ST, SST, SRA, SCM = 88, 89, 90, 92, 94
    # options
    FEATURES = False       # (no softcap / ALiBi pass in this body)
    LEFTWIN = False        # (no left windows: the one-sided key limit)
    DMAMIX = True
    # parameters (gen_fwdpp.PingPong explains them)
    RING, DLEAD, NPIECE, EPI_SCALE = 4, 3, 4, None
    XDL_NOPS = ["s_nop 7", "s_nop 7", "s_nop 3"]
    VPH_NOPS = ["s_nop 7", "s_nop 7"]
    N_EPI_STORES = 18      # 16 O stores (8 bytes) + 2 LSE stores

    SIG = ("const int kblo, const int kbhi, const int vblo, const int vbhi, const int kvbytes, "
           "const i32x4 qsrd, const i32x4 osrd, const i32x4 lsrd, const int kstep, const int kdst, "
           "const int ntl, const int tw, const int ew, const int grp, const float c, const float thr, "
           "const int kb0, const int vb0, const int vb1, const int dma0, const int dma1, "
           "const int lim0, const int lim1, const int qoff0, const int qoff1, const int ooff0, "
           "const int ooff1, const int loff0, const int loff1")
    INS = (asmgen.operands("s", "kblo kbhi vblo vbhi kvbytes qsrd osrd lsrd kstep kdst ntl tw ew grp c thr") +
           asmgen.operands("v", "kb0 vb0 vb1 dma0 dma1 lim0 lim1 qoff0 qoff1 ooff0 ooff1 loff0 loff1"))

    def nvgpr(self):
        return self.MISC + 8

    def otup(self, dt, rt):
        b = self.ABASE_O + 4 * (2 * dt + rt)
        return f"a[{b}:{b + 3}]"

    def qtup(self, rt, s):
        b = self.ABASE_Q + 4 * (4 * rt + s)
        return f"a[{b}:{b + 3}]"

    def sv(self, kt, rt):
        b = self.SBASE + 4 * (2 * kt + rt)
        return f"v[{b}:{b + 3}]"

    def ptup(self, ks, rt):
        b = self.PBASE + 4 * (2 * ks + rt)
        return f"v[{b}:{b + 3}]"

    def value_info(self, v):
        """score v = 8 kt + 4 rt + r of this lane (its S register): key offset in the tile minus
        4 g, its row tile, P dword (pairs r, r + 1)"""
        kt, rt, r = v // 8, (v // 4) % 2, v % 4
        return 16 * kt + r, rt, self.PBASE + 4 * (2 * (kt // 2) + rt) + 2 * (kt % 2) + r // 2

    def k_read(self, f, slot_tile, dst_slot):
        s, kt = f // 4, f % 4
        return f"ds_read_b128 {self.ktup(dst_slot)}, %[kb0] offset:{slot_tile * self.TILE + 4096 * kt + 512 * s}"

    def v_reads(self, f, slot_tile, dst_slot):
        ks, dt = f // 8, f % 8
        off = slot_tile * self.TILE + 8192 * ks + 512 * (dt >> 1)   # (the lane base carries the V ring)
        return [f"ds_read_b64_tr_b16 {self.vtup(dst_slot, h)}, %[vb{dt & 1}] offset:{off + 4096 * h}"
                for h in (0, 1)]

    def mfmas(self, dt, pv, qk):
        """PV(j) then QK^T(j+1), 16 fragments each; a K / V^T fragment feeds the MFMAs of both row
        tiles (gen_fwdpp.PingPong.m_phase places the reads around this list)"""
        mnem = "v_mfma_f32_16x16x32_" + dt
        mf = []
        if pv:
            for f in range(16):
                ks, d = f // 8, f % 8
                for rt in (0, 1):
                    mf.append((("V", f), f"{mnem} {self.otup(d, rt)}, {self.vtup(f % self.VS)}, "
                                         f"{self.ptup(ks, rt)}, {self.otup(d, rt)}"))
        if qk:
            for f in range(16):
                s, kt = f // 4, f % 4
                for rt in (0, 1):
                    src = self.sv(kt, rt) if s else "0"
                    mf.append((("K", f), f"{mnem} {self.sv(kt, rt)}, {self.ktup(f % self.KS)}, "
                                         f"{self.qtup(rt, s)}, {src}"))
        return mf

    def softmax(self, dt, mask):
        """P = exp2(S c - m_rt) of this lane's 32 scores (2 rows x 16 keys; masked: keys at or past
        the row's limit give 0), the rows' tile sums in LT, LT + 1; 4 scores in flight"""
        LT, TMP = self.LT, self.TMP
        stages = []
        started = [False, False]
        for v in range(32):
            t = f"v{TMP + v % 8}"
            off, rt, dword = self.value_info(v)
            ex = [f"v_exp_f32 {t}, {t}"]
            if mask:
                ex += [f"v_cmp_lt_i32 vcc, {off}, v{self.LIM + rt}", f"v_cndmask_b32 {t}, 0, {t}, vcc"]
            acc = (f"v_add_f32 v{LT + rt}, v{LT + rt}, {t}" if started[rt] else f"v_mov_b32 v{LT + rt}, {t}")
            started[rt] = True
            st = [[f"v_fma_f32 {t}, v{self.SBASE + v}, %[c], v{self.NM + rt}"], ex, [acc]]
            if v & 1:
                st[2].append(f"v_cvt_pk_{dt}_f32 v{dword}, v{TMP + (v - 1) % 8}, {t}")
            stages.append(st)
        return asmgen.stagger(stages) + ["s_nop 0"]

    def row_reduce(self, op, dst, t2):
        """dst = op over the 4 lanes l16 + 16 g of this lane's row (permlane32 then permlane16)"""
        return [f"v_mov_b32 {t2}, {dst}", "s_nop 1", f"v_permlane32_swap_b32 {dst}, {t2}", "s_nop 1",
                f"{op} {dst}, {dst}, {t2}", f"v_mov_b32 {t2}, {dst}", "s_nop 1",
                f"v_permlane16_swap_b32 {dst}, {t2}", "s_nop 1", f"{op} {dst}, {dst}, {t2}"]

    def row_max2(self, dst0, dst1):
        """masked max of each of the lane's two rows over the tile's 64 keys -> dst0, dst1"""
        t2, ninf = f"v{self.MISC + 2}", f"v{self.MISC + 5}"
        dst = (dst0, dst1)
        out = [f"v_mov_b32 {ninf}, 0xff800000", f"v_mov_b32 {dst0}, {ninf}", f"v_mov_b32 {dst1}, {ninf}"]
        for v in range(32):
            off, rt, _ = self.value_info(v)
            out += [f"v_cmp_lt_i32 vcc, {off}, v{self.LIM + rt}",
                    f"v_cndmask_b32 {t2}, {ninf}, v{self.SBASE + v}, vcc",
                    f"v_max_f32 {dst[rt]}, {dst[rt]}, {t2}"]
        return out + self.row_reduce("v_max_f32", dst0, t2) + self.row_reduce("v_max_f32", dst1, t2)

    def first_max(self, uid):
        """m_rt = the masked max of tile 0 per row (NM = -c max, 0 for a row with no key)"""
        mx, t2 = f"v{self.MISC}", f"v{self.MISC + 2}"
        out = self.XDL_NOPS + self.row_max2(mx, f"v{self.MISC + 1}")
        for rt in (0, 1):
            m = f"v{self.MISC + rt}"
            out += [f"v_mul_f32_e64 {t2}, -%[c], {m}", f"v_cmp_lg_f32 vcc, 0xff800000, {m}",
                    f"v_cndmask_b32 v{self.NM + rt}, 0, {t2}, vcc"]
        return out

    def redo_block(self, dt, uid):
        """rare path (gen_fwdpp's redo_block per row): the tile's true masked max per row, m_new =
        max(m, c max); the row's O and l scaled by 2^(m - m_new); the softmax redone"""
        MISC, NM, LRUN = self.MISC, self.NM, self.LRUN
        out = [f".Lredo_{uid}:"] + self.XDL_NOPS + self.row_max2(f"v{MISC}", f"v{MISC + 1}")
        t2 = f"v{MISC + 2}"
        alpha = (f"v{MISC + 3}", f"v{MISC + 4}")
        for rt in (0, 1):
            mx = f"v{MISC + rt}"
            out += [f"v_mul_f32 {t2}, %[c], {mx}",
                    f"v_max_f32_e64 {t2}, {t2}, -v{NM + rt}",
                    f"v_add_f32 {alpha[rt]}, v{NM + rt}, {t2}",
                    f"v_exp_f32_e64 {alpha[rt]}, -{alpha[rt]}",
                    f"v_mul_f32 v{NM + rt}, -1.0, {t2}",
                    "s_nop 0",
                    f"v_mul_f32 v{LRUN + rt}, v{LRUN + rt}, {alpha[rt]}"]
        for i in range(64):
            t = f"v{self.TMP + i % 8}"
            rt = (i // 4) % 2
            out += [f"v_accvgpr_read_b32 {t}, a{self.ABASE_O + i}", f"v_mul_f32 {t}, {t}, {alpha[rt]}",
                    f"v_accvgpr_write_b32 a{self.ABASE_O + i}, {t}"]
        out += ["s_nop 1"] + self.softmax(dt, True)
        return out + ["s_nop 3", f"s_setpc_b64 s[{self.SRA}:{self.SRA + 1}]"]

    def redo_test(self):
        """vcc = either row's tile sum on any lane past 2^slack"""
        t = f"v{self.MISC + 2}"
        return [f"v_max_f32 {t}, v{self.LT}, v{self.LT + 1}", f"v_cmp_lt_f32 vcc, %[thr], {t}"]

    def lrun_add(self):
        return [f"v_add_f32 v{self.LRUN + rt}, v{self.LRUN + rt}, v{self.LT + rt}" for rt in (0, 1)]

    def lim_step(self):
        return [f"v_add_u32 v{self.LIM + rt}, -64, v{self.LIM + rt}" for rt in (0, 1)]

    def epilogue_core(self, dt):
        """per row: the sums of its 4 lanes combined, O / l -> dt (4 consecutive d per lane: 8-byte
        stores), LSE by the g = 0 lanes (loff is out of range on the others)"""
        T = self.TMP
        inv = (f"v{T + 6}", f"v{T + 7}")
        out = []
        for rt in (0, 1):
            L, t, lse, cls, pinf = (f"v{T + i}" for i in range(5))
            out += [f"v_mov_b32 {pinf}, 0x7f800000", f"v_mov_b32 {L}, v{self.LRUN + rt}"]
            out += self.row_reduce("v_add_f32", L, t)
            out += [f"v_rcp_f32 {inv[rt]}, {L}", f"v_log_f32 {lse}, {L}",
                    f"v_mov_b32 {cls}, 0x63", f"v_cmp_class_f32 vcc, {L}, {cls}",
                    f"v_cndmask_b32_e64 {inv[rt]}, {inv[rt]}, 1.0, vcc",
                    f"v_sub_f32 {lse}, {lse}, v{self.NM + rt}",
                    f"v_mul_f32 {lse}, 0x3f317218, {lse}", f"v_cndmask_b32 {lse}, {lse}, {pinf}, vcc",
                    f"buffer_store_dword {lse}, %[loff{rt}], %[lsrd], 0 offen"]
        for d in range(8):
            for rt in (0, 1):
                vb = 8 * ((2 * d + rt) % 4)                 # four rotating register sets in S
                vals = [f"v{vb + k}" for k in range(4)]
                src = [f"a{self.ABASE_O + 4 * (2 * d + rt) + k}" for k in range(4)]
                out += [f"v_accvgpr_read_b32 {vals[k]}, {src[k]}" for k in range(4)]
                out += [f"v_mul_f32 {vals[k]}, {vals[k]}, {inv[rt]}" for k in range(4)]
                out += [f"v_cvt_pk_{dt}_f32 v{vb + 4 + k}, {vals[2 * k]}, {vals[2 * k + 1]}" for k in range(2)]
                out += [f"buffer_store_dwordx2 v[{vb + 4}:{vb + 5}], %[ooff{rt}], %[osrd], 0 offen offset:{32 * d}"]
        return out

    def item_program(self, dt):
        out = (asmgen.STAMP_INIT if self.STAMPS else []) + ["s_waitcnt lgkmcnt(0)"]
        for rt in (0, 1):
            out += [f"v_mov_b32 v{self.NM + rt}, 0", f"v_mov_b32 v{self.LRUN + rt}, 0",
                    f"v_mov_b32 v{self.LIM + rt}, %[lim{rt}]"]
        out += [f"s_mov_b32 s{self.SST}, 0"]
        out += [f"buffer_load_dwordx4 {self.qtup(rt, s)}, %[qoff{rt}], %[qsrd], 0 offen offset:{64 * s}"
                for rt in (0, 1) for s in range(4)]
        out += [f"v_accvgpr_write_b32 a{self.ABASE_O + i}, 0" for i in range(64)]
        out += self.dense_descriptors()
        for slot in range(self.DLEAD - 1):                       # tiles 0 .. DLEAD-2
            out += sum(self.dma_pieces(slot), []) + self.dma_advance()
        out += [f"s_waitcnt vmcnt({self.NPIECE * (self.DLEAD - 2)})", "s_barrier"]   # Q and tile 0 landed
        return out + self.groups(dt)


def emit(out=OUT, **options):
    """options: stamps, lead"""
    body = PingPong16(**options)
    asmgen.write_header(
        out, "gen_fwdpp16.py",
        ["// The 8-wave ping-pong D = 128 forward's item body on v_mfma_f32_16x16x32 (fmha_fwdpp_kernel.h,",
         "// M16): one asm statement per dtype with a fixed register map; see the generator's docstring."],
        [ln for dt in ("bf16", "f16") for ln in body.function(dt)],
        defines=["#define XFA_FWDPP16_STAMPS 1         // diagnostic build (--stamps)"] if body.STAMPS else [],
        decls=[f"constexpr int kFwdpp16Ring = {body.RING};         // K / V tile slots the body addresses"])


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--lead", type=int, default=PingPong16.LEAD)
    ap.add_argument("--stamps", action="store_true", help="diagnostic phase stamps")
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    emit(a.out, stamps=a.stamps, lead=a.lead)
