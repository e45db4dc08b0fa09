"""LDS bank cycles of every per-tile LDS instruction of the MLA decode kernel
(fmha_mla_decode_kernel.h) under its image, byte (row, chunk) at row * 1152 + 16 (chunk ^ (row & 6)),
against the same image without the XOR.  Lane groups and bank functions as tools/decode_banks.py
(MI355X_MICROARCH.md § LDS): ds_read_b128 4 groups of 16 (64 banks), ds_read_b64_tr_b16 2 x 32
(64 banks), ds_write_b128 8 x 8 contiguous lanes (32 banks).

  python tools/mla_banks.py

The fp8-cache kernel (fmha_mla_decode_fp8_kernel.h) reads the same image with the same
instructions; its 36 image writes per tile (per 16-row half: 8 latent loads x 2 ds_write_b128, 2
rotary loads x 1) are checked here too, against the order in which every lane writes its even chunk
first.  Its descales move with ds_bpermute_b32, which addresses no LDS memory and has no banks.

The 1152-byte pitch is 4.5 bank rows of 256 B: odd rows sit half a bank row on, and the XOR with
row & 6 (period 8 rows, inside the aligned 8-chunk blocks of a 72-chunk row) spreads the even and
the odd rows over the eight 16-byte slots of their half.
"""
from decode_banks import B128, HALVES, W8, cycles

PITCH, CPR = 1152, 72


def mla_off(r, c):
    return r * PITCH + ((c ^ (r & 6)) << 4)


def linear(r, c):
    return r * PITCH + (c << 4)


def k_reads(off):
    """S^T row reads: k-step s, key block kb; lane l reads row 16 kb + l % 16, chunk 4 s + l / 16."""
    return [cycles([off(16 * kb + (l & 15), 4 * s + (l >> 4)) for l in range(64)], B128, 16, 64)
            for s in range(18) for kb in range(2)]


def v_reads(off):
    """O^T transposed reads over the first 512 columns: d tile dt, part; lane l reads 8 bytes of
    row 4 (l / 16) + (l % 16) / 4 + 16 part at column 16 dt + 4 (l % 4)."""
    out = []
    for part in range(2):
        for dt in range(32):
            ad = []
            for l in range(64):
                r = 4 * (l >> 4) + ((l & 15) >> 2) + 16 * part
                col = 16 * dt + 4 * (l & 3)
                ad.append(off(r, col >> 3) + 8 * ((col >> 2) & 1))
            out.append(cycles(ad, HALVES, 8, 64))
    return out


def writes(off):
    """Image writes: instruction i of a 16-row half tile h; lane l writes chunk f = 64 i + l of the
    half's contiguous run: row 16 h + f / 72, chunk f % 72."""
    return [cycles([off(16 * h + (64 * i + l) // CPR, (64 * i + l) % CPR) for l in range(64)], W8, 16, 32)
            for h in range(2) for i in range(18)]


def writes8(swap):
    """The fp8 kernel's image writes of a half tile.  Latent load i, lane l: row 2 i + l / 32, latent
    chunk c = l % 32 -> image chunks 2 c and 2 c + 1, one ds_write_b128 each; swap: lanes with bit 2
    set write the odd chunk first (the kernel), else every lane the even one.  Rotary load j, lane
    l: row 8 j + l / 8 -> image chunk 64 + l % 8.  Also checks the kernel's address forms."""
    out, cover = [], set()
    for i in range(8):
        first, second = [], []
        for l in range(64):
            r, c, odd = 2 * i + (l >> 5), l & 31, ((l >> 2) & 1 if swap else 0)
            first.append(mla_off(r, 2 * c + odd))
            second.append(mla_off(r, 2 * c + 1 - odd))
            wl = (l >> 5) * PITCH + 16 * ((2 * c + odd) ^ (2 * (i & 3)))        # the kernel's wl[i % 4]
            assert first[-1] == 2 * i * PITCH + wl and second[-1] == 2 * i * PITCH + (wl ^ 16)
        cover.update(first + second)
        out += [cycles(first, W8, 16, 32), cycles(second, W8, 16, 32)]
    for j in range(2):
        ad = [mla_off(8 * j + (l >> 3), 64 + (l & 7)) for l in range(64)]
        for l in range(64):
            assert ad[l] == 8 * j * PITCH + (l >> 3) * PITCH + 16 * ((64 + (l & 7)) ^ ((l >> 3) & 6))   # wr
        cover.update(ad)
        out.append(cycles(ad, W8, 16, 32))
    assert sorted(cover) == list(range(0, 16 * PITCH, 16))      # every chunk of the 16 rows, once
    return out


def report8():
    plain, swapped = writes8(False), writes8(True)
    print(f"fp8 image writes per half tile (18 ds_write_b128): even chunk first {sum(plain) / len(plain):.2f} "
          f"max {max(plain)};  bit 2 of the lane swaps {sum(swapped) / len(swapped):.2f} max {max(swapped)} (8)")
    return max(swapped)


def report(name, off):
    k, v, w = k_reads(off), v_reads(off), writes(off)
    print(f"{name:8s} K ds_read_b128 {sum(k) / len(k):.2f} max {max(k)} (4 ideal)   V ds_read_b64_tr_b16 "
          f"{sum(v) / len(v):.2f} max {max(v)} (2)   ds_write_b128 {sum(w) / len(w):.2f} max {max(w)} (8)")
    return max(k), max(v), max(w)


if __name__ == "__main__":
    report("linear", linear)
    worst = report("mla_off", mla_off)
    assert worst == (4, 2, 8), worst
    # the image is a bijection of the tile's 32 x 72 chunks onto its 36,864 bytes
    assert sorted(mla_off(r, c) for r in range(32) for c in range(CPR)) == list(range(0, 32 * PITCH, 16))
    # the address forms the kernel uses (two registers for the row reads, four for the transposed)
    for l in range(64):
        lr, hh = l & 15, l >> 4
        b = (lr >> 2) & 1
        base = lr * PITCH + 16 * (hh ^ (lr & 2))
        for s in range(18):
            assert mla_off(lr, 4 * s + hh) == (base - 64 * b if s & 1 else base + 64 * b) + 64 * s
        vrow = 4 * hh + ((l & 15) >> 2)
        for dt in range(32):
            col = 16 * dt + 4 * (l & 3)
            want = mla_off(vrow, col >> 3) + 8 * ((col >> 2) & 1)
            got = vrow * PITCH + 32 * ((dt & 3) ^ ((vrow >> 1) & 3)) + 16 * ((l >> 1) & 1) + 8 * (l & 1) + 128 * (dt >> 2)
            assert want == got
    print("conflict-free: every K read 4 cycles, every V read 2, every write 8; address forms verified")
    assert report8() == 8
    print("fp8 kernel: every image write 8 cycles; address forms verified")
