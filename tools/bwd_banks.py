"""LDS bank cycles of the backward's dS^T traffic (D = 128: 8 waves x 32 keys): the bf16 dS^T
stores (ds_write_b64, 4 groups of 16 contiguous lanes, 32 banks) and the dQ phase's
transposed reads (ds_read_b64_tr_b16, 2 x 32 lanes, 64 banks), under round 3's image and the
current fmha_bwd_kernel.h ds_off (lane groups: MI355X_MICROARCH.md § LDS).  And, first, the MLA
backward's four kv_off tiles (fmha_bwd_mla_kernel.h): row reads, transposing reads, loader stores.

  python tools/bwd_banks.py
"""


def round3(row, col):
    return row * 64 + (((col >> 3) ^ (((row >> 3) & 1) << 1)) << 4) + ((col >> 2) & 1) * 8


def current(row, col):
    s1 = (((row >> 3) & 1) << 1) | ((row >> 1) & 1)
    s0 = (row >> 2) & 1
    return row * 64 + (((col >> 3) ^ s1) << 4) + ((((col >> 2) & 1) ^ s0) << 3)


def cycles(addrs, groups, width, nbanks):
    tot = 0
    for g in groups:
        banks = {}
        for lane in g:
            a = addrs[lane]
            for w in range(width // 4):
                banks.setdefault((a // 4 + w) % nbanks, set()).add(a // width)
        tot += max(len(v) for v in banks.values())
    return tot


def kv_off(hd, row, chunk):
    """fmha_common.h kv_off<HD>: the image of the MLA backward's Q / dO and K / V tiles"""
    return (hd * 16) * (row >> 3) + 512 * (chunk >> 2) + 64 * (row & 7) + 16 * ((chunk & 3) ^ ((row >> 2) & 3))


# ds_read_b128 is serviced in these four groups of 16 lanes (MI355X_MICROARCH.md § LDS)
B128_GROUPS = [[0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27],
               [4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31]]
B128_GROUPS += [[l + 32 for l in g] for g in B128_GROUPS]


def mla():
    """The MLA backward (fmha_bwd_mla_kernel.h), widths 192 and 128: the row reads (ds_read_b128,
    lane = row lane & 31, chunk 2 s + (lane >> 5)), the transposing reads (ds_read_b64_tr_b16:
    row 8 part + 4 (lane >> 5) + ((lane & 15) >> 2), column 32 dt + 16 ((lane >> 4) & 1) + 4 (lane
    & 3)) and the loaders' ds_write_b128 (thread t: chunk t + 256 j, 8 groups of 8 contiguous
    lanes, 32 banks) of a `rows`-row tile."""
    for hd, rows, what in ((192, 32, "Q tile"), (128, 32, "dO tile"), (192, 64, "K tile"), (128, 64, "V tile")):
        cpr = hd // 8
        rd = [cycles([kv_off(hd, r0 + (l & 31), 2 * s + (l >> 5)) for l in range(64)], B128_GROUPS, 16, 64)
              for r0 in range(0, rows, 32) for s in range(hd // 16)]
        def tr_addr(l, r0, part, dt):
            col = 32 * dt + 16 * ((l >> 4) & 1) + 4 * (l & 3)
            return kv_off(hd, r0 + 8 * part + 4 * (l >> 5) + ((l & 15) >> 2), col >> 3) + 8 * ((col >> 2) & 1)

        tr = [cycles([tr_addr(l, r0, part, dt) for l in range(64)], [list(range(32)), list(range(32, 64))], 8, 64)
              for r0 in range(0, rows, 16) for part in range(2) for dt in range(hd // 32)]
        wr = [cycles([kv_off(hd, (t + 256 * j) // cpr, (t + 256 * j) % cpr) for t in range(64 * w, 64 * w + 64)],
                     [list(range(8 * g, 8 * g + 8)) for g in range(8)], 16, 32)
              for j in range(rows * cpr // 256) for w in range(4)]
        print(f"MLA {what:8s} [{rows}][{hd}]  ds_read_b128 {sum(rd) / len(rd):.1f} cycles (4 ideal)   "
              f"ds_read_b64_tr_b16 {sum(tr) / len(tr):.1f} (2 ideal)   ds_write_b128 {sum(wr) / len(wr):.1f} (8 ideal)")


if __name__ == "__main__":
    mla()
    for name, f in (("round 3", round3), ("current", current)):
        st = [cycles([f(w * 32 + (l & 31), 8 * gq + 4 * (l >> 5)) for l in range(64)],
                     [list(range(16 * j, 16 * j + 16)) for j in range(4)], 8, 32)
              for w in range(8) for gq in range(4)]
        rd = [cycles([ks * 32 * 64 + f(8 * (l >> 4) + ((l & 15) >> 2) + 4 * part, 16 * mt + 4 * (l & 3))
                      for l in range(64)], [list(range(32)), list(range(32, 64))], 8, 64)
              for mt in range(2) for part in range(2) for ks in range(8)]
        for r in range(64):
            assert sorted((f(r, c) - r * 64) // 8 for c in range(0, 32, 4)) == list(range(8))
        print(f"{name:8s} dS^T ds_write_b64 {sum(st) / len(st):.1f} cycles (4 ideal)   "
              f"dQ ds_read_b64_tr_b16 {sum(rd) / len(rd):.1f} (2 ideal)")
