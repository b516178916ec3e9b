#!/usr/bin/env python3
"""CPU check of the LDS images of corrla_rs_amd/csrc/mixed_kernels.hpp (no GPU needed): replays, with the same formulas,
what the loader waves' LDS-DMA writes (physical 16-byte slot <- logical slot, rule 21 of cdna_hip_programming.md: linear
destination, swizzled SOURCE) and what the MFMA waves read back, and verifies
  * every fragment read returns the reduction indices kmap(g, j) of the right row / column, for both kernels and all
    planes / column tiles / row tiles,
  * every ds_read_b128 (four 16-lane groups, MI355X_MICROARCH.md LDS table) and ds_read_b32 (two 32-lane groups) of the
    kernels is bank-conflict free,
  * split_planes_kernel's position -> reduction index map equals the fragment order the big operand is read in.
and the same for the two images of corrla_rs_amd/csrc/bf16in_kernels.hpp (big operand stored in bf16, 16-KiB tiles): the
ds_read_b128 of the nn image, the two ds_read_b64_tr_b16 of the tn image (addresses 8-byte aligned, the 4 x 16 block each
16-lane group gathers, conflict freedom per 32-lane half on 64 banks) and the identity reduction map of its planes.
Run: python tools/lds_layout_check.py"""
import itertools
import sys

KT, BIG, OUTER = 32, 32768, 256
B128_GROUPS = [list(range(0, 4)) + list(range(12, 16)) + list(range(20, 28)),
               list(range(4, 12)) + list(range(16, 20)) + list(range(28, 32)),
               list(range(32, 36)) + list(range(44, 48)) + list(range(52, 60)),
               list(range(36, 44)) + list(range(48, 52)) + list(range(60, 64))]


def kmap(p):
    return 16 + 4 * (p >> 3) + (p & 3) if (p & 4) else 4 * (p >> 3) + (p & 3)


def big_swz(row):
    return (row >> 1) & 7


def plane_swz(row):
    return (-(row >> 2)) & 3


def tn_swz(kr):
    return ((kr >> 2) & 1) << 2


def fill_stage(nt, np_, tn):
    """LDS 16-byte slot index -> what it holds after the DMA of one tile."""
    lds = {}
    plane = nt * 16 * KT * 2
    for c in range(BIG // 1024):
        for lane in range(64):
            dst = (c * 1024 + 16 * lane) // 16
            if not tn:
                row = 8 * c + (lane >> 3)
                ls = (lane & 7) ^ big_swz(row)
                lds[dst] = ("big", row, tuple(4 * ls + e for e in range(4)))       # outer row, reduction indices
            else:
                kr = c
                ls = lane ^ tn_swz(kr)
                lds[dst] = ("big", kr, tuple(4 * ls + e for e in range(4)))        # reduction row, outer columns
    for p in range(np_):
        for ct in range(nt):
            for lane in range(64):
                row = 16 * ct + (lane >> 2)
                ls = (lane & 3) ^ plane_swz(row)
                dst = (BIG + p * plane + ct * 1024 + 16 * lane) // 16
                lds[dst] = ("plane", p, row, tuple(kmap(8 * ls + j) for j in range(8)))  # column, reduction indices held
    return lds, plane


def conflict_free_b128(addrs):
    for grp in B128_GROUPS:
        slots = {}
        for lane in grp:
            s = (addrs[lane] // 16) % 16
            if s in slots and slots[s] != addrs[lane]:
                return False
            slots[s] = addrs[lane]
    return True


def conflict_free_b32(addrs):
    for grp in (range(0, 32), range(32, 64)):
        banks = {}
        for lane in grp:
            b = (addrs[lane] // 4) % 32
            if b in banks and banks[b] != addrs[lane]:
                return False
            banks[b] = addrs[lane]
    return True


def check(nt, np_, tn):
    lds, plane = fill_stage(nt, np_, tn)
    want_k = [[kmap(8 * g + j) for j in range(8)] for g in range(4)]
    for wave, mw in itertools.product(range(8), range(2)):
        if not tn:
            for half in range(2):
                addrs = {}
                for lane in range(64):
                    fr, fg = lane & 15, lane >> 4
                    a_base = (32 * wave + fr) * 128 + ((fg ^ big_swz(fr)) << 4)
                    addr = (a_base + mw * 2048) ^ (64 * half)
                    addrs[lane] = addr
                    kind, row, ks = lds[addr // 16]
                    assert kind == "big" and row == 32 * wave + 16 * mw + fr, (wave, mw, lane, row)
                    assert list(ks) == want_k[fg][4 * half:4 * half + 4], (lane, ks)
                assert conflict_free_b128(addrs), ("nn big", wave, mw, half)
        else:
            for j in range(8):
                addrs = {}
                for lane in range(64):
                    fr, fg = lane & 15, lane >> 4
                    a_base = (((32 * wave + fr) >> 2) << 4) + ((fr & 3) << 2)
                    off = (a_base + mw * 64) ^ ((fg & 1) << 6)
                    kr = 4 * fg + (j if j < 4 else 12 + j)
                    assert kr == want_k[fg][j]
                    addr = kr * 1024 + off
                    addrs[lane] = addr
                    kind, row, cols = lds[addr // 16]
                    assert kind == "big" and row == kr, (lane, j, row, kr)
                    assert cols[(addr % 16) // 4] == 32 * wave + 16 * mw + fr, (lane, j, cols, addr)
                assert conflict_free_b32(addrs), ("tn big", wave, mw, j)
    for t, p in itertools.product(range(nt), range(np_)):
        addrs = {}
        for lane in range(64):
            fr, fg = lane & 15, lane >> 4
            b_base = BIG + fr * 64 + ((fg ^ plane_swz(fr)) << 4)
            addr = b_base + t * 1024 + p * plane
            addrs[lane] = addr
            kind, pp, col, ks = lds[addr // 16]
            assert kind == "plane" and pp == p and col == 16 * t + fr, (t, p, lane, pp, col)
            assert list(ks) == want_k[fg], (lane, ks)
        assert conflict_free_b128(addrs), ("plane", t, p)


# ---- bf16in_kernels.hpp ----------------------------------------------------------------------------------------------
BA_BIG = 16384


def ba_tn_swz(kr):
    return (kr & 3) | ((kr >> 1) & 4)


def ba_fill_big(tn):
    """LDS 16-byte slot index -> (row, the 8 element indices along the row) after the DMA of one big tile."""
    lds = {}
    for c in range(BA_BIG // 1024):
        for lane in range(64):
            dst = (c * 1024 + 16 * lane) // 16
            if not tn:
                row = 16 * c + (lane >> 2)
                ls = (lane & 3) ^ plane_swz(row)
                lds[dst] = (row, tuple(8 * ls + e for e in range(8)))                 # outer row, reduction indices
            else:
                kr = 2 * c + (lane >> 5)
                sp = lane & 31
                lb = (sp >> 1) ^ ba_tn_swz(kr)
                lds[dst] = (kr, tuple(16 * lb + 8 * (sp & 1) + e for e in range(8)))  # reduction row, outer columns
    assert len(lds) == BA_BIG // 16
    return lds


def conflict_free_b64(addrs):
    """ds_read_b64 / ds_read_b64_tr_b16: 64 banks of 4 bytes, the two 32-lane halves"""
    for grp in (range(0, 32), range(32, 64)):
        banks = {}
        for lane in grp:
            for d in range(2):
                b = (addrs[lane] // 4 + d) % 64
                if b in banks and banks[b] != addrs[lane] // 4 + d:
                    return False
                banks[b] = addrs[lane] // 4 + d
    return True


def check_bf16a(tn):
    lds = ba_fill_big(tn)
    for wave, mw in itertools.product(range(8), range(2)):
        if not tn:
            addrs = {}
            for lane in range(64):
                fr, fg = lane & 15, lane >> 4
                addr = (32 * wave + 16 * mw + fr) * 64 + ((fg ^ plane_swz(fr)) << 4)
                addrs[lane] = addr
                row, ks = lds[addr // 16]
                assert row == 32 * wave + 16 * mw + fr, (wave, mw, lane, row)
                assert list(ks) == [8 * fg + j for j in range(8)], (lane, ks)       # identity reduction map
            assert conflict_free_b128(addrs), ("bf16a nn", wave, mw)
        else:
            for half in range(2):
                addrs = {}
                for lane in range(64):
                    fr, fg = lane & 15, lane >> 4
                    kr = 8 * fg + (fr >> 2)
                    addr = kr * 512 + (((2 * wave + mw) ^ ba_tn_swz(kr)) << 5) + ((fr & 3) << 3) + half * 4 * 512
                    assert addr % 8 == 0 and addr + 8 <= BA_BIG
                    addrs[lane] = addr
                # the hardware transpose: lane 4 q + p of a 16-lane group supplies row q, columns 4 p .. 4 p + 3 of the block;
                # lane i receives column i of the four rows, row q in element q
                for lane in range(64):
                    fr, fg = lane & 15, lane >> 4
                    for q in range(4):
                        src = addrs[16 * fg + 4 * q + (fr >> 2)]
                        row, cols = lds[src // 16]
                        col = cols[(src % 16) // 2 + (fr & 3)]
                        assert row == 8 * fg + 4 * half + q, (lane, q, row)        # reduction index 8 g + j, j = 4 half + q
                        assert col == 32 * wave + 16 * mw + fr, (lane, q, col)
                assert conflict_free_b64(addrs), ("bf16a tn", wave, mw, half)


def check_bf16a_planes(nt):
    """plane images as in check(), filled by split_planes_kernel<3, false>: position q of a column holds reduction index q"""
    plane = nt * 16 * KT * 2
    lds = {}
    for p, ct, lane in itertools.product(range(3), range(nt), range(64)):
        row = 16 * ct + (lane >> 2)
        ls = (lane & 3) ^ plane_swz(row)
        lds[(p * plane + ct * 1024 + 16 * lane) // 16] = (p, row, tuple(8 * ls + j for j in range(8)))
    for t, p in itertools.product(range(nt), range(3)):
        addrs = {}
        for lane in range(64):
            fr, fg = lane & 15, lane >> 4
            addr = fr * 64 + ((fg ^ plane_swz(fr)) << 4) + t * 1024 + p * plane
            addrs[lane] = addr
            pp, col, ks = lds[addr // 16]
            assert pp == p and col == 16 * t + fr and list(ks) == [8 * fg + j for j in range(8)], (t, p, lane)
        assert conflict_free_b128(addrs), ("bf16a plane", t, p)


if __name__ == "__main__":
    assert sorted(kmap(p) for p in range(32)) == list(range(32))
    n = 0
    for nt, np_, tn in itertools.product(range(1, 10), (2, 3), (False, True)):
        check(nt, np_, tn)
        n += 1
    print(f"{n} kernel variants: fragment maps and bank-conflict freedom OK")
    for tn in (False, True):
        check_bf16a(tn)
    for nt in range(1, 10):
        check_bf16a_planes(nt)
    print("bf16-input kernel: nn / tn big images and plane images for NT = 1..9 OK")
