"""LDS bank cycles of the per-stage LDS instructions of the ragged index logits kernel
(fmha_mla_index_ragged_kernel.h) under its image, byte (row, chunk) at row * 128 + 16 (chunk ^
(row / 2 % 8)) (k8_off), against the same image without the XOR.  Lane groups and bank functions as
tools/decode_banks.py: ds_read_b128 4 groups of 16 (64 banks), ds_write_b128 8 x 8 contiguous lanes
(32 banks).

  python tools/mla_index_ragged_banks.py

A stage is 128 key rows of 128 bytes.  Read: tile tt, step c; lane l reads row 32 tt + l % 32, chunk
4 (l / 32) + c.  Write: piece j * threads + t of the stage is (row piece / 8, chunk piece % 8).
Why it works: rows m and m + 2 are 256 bytes apart, one bank row; the 16 lanes of a read group hold
8 even and 8 odd rows whose m / 2 % 8 are all different, and the XOR sends them to the 8 different
16-byte slots of their half bank row.
"""
from decode_banks import B128, W8, cycles


def k8_off(r, c):
    return r * 128 + ((c ^ ((r >> 1) & 7)) << 4)


def linear(r, c):
    return r * 128 + (c << 4)


def reads(off):
    return [cycles([off(32 * tt + (l & 31), 4 * (l >> 5) + c) for l in range(64)], B128, 16, 64)
            for tt in range(4) for c in range(4)]


def writes(off, threads):
    return [cycles([off((j * threads + 64 * w + l) >> 3, l & 7) for l in range(64)], W8, 16, 32)
            for j in range(1024 // threads) for w in range(threads // 64)]


if __name__ == "__main__":
    for name, off in (("linear", linear), ("k8_off", k8_off)):
        r, w4, w8 = reads(off), writes(off, 256), writes(off, 512)
        print(f"{name:7s} B ds_read_b128 {sum(r) / len(r):.2f} max {max(r)} (4 ideal)   ds_write_b128 "
              f"{sum(w4) / len(w4):.2f} max {max(w4)} / 8 waves {max(w8)} (8)")
    assert max(reads(k8_off)) == 4 and max(writes(k8_off, 256)) == 8 and max(writes(k8_off, 512)) == 8
    assert sorted(k8_off(r, c) for r in range(128) for c in range(8)) == list(range(0, 128 * 128, 16))
    print("conflict-free: every B read 4 cycles, every write 8; the image is a bijection of the stage")
