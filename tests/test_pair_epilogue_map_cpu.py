"""The staged epilogue 2 of the resblock pair kernel, replayed on the CPU.

csrc/resblock_cl.hip (STAGED) sends each wave's WM x WN accumulator tile
through a wave-private f32 LDS tile, CW = min(WN, 64) columns per pass:

    write   (wave, lane, mi, nj, rg) -> St[wave][(mi*16 + kl*4 + rg)*SP
                                                 + nj*16 + il]
            kl = lane >> 4, il = lane & 15, SP = CW + 4 floats
    read    (wave, lane, g)          -> row g*RPP + lane // LPR,
                                        floats (lane % LPR)*8 .. +7
            LPR = CW/8 lanes per row, RPP = 64/LPR rows per read
    global  row t0 + wr*WM + row, channels wc*WN + h*CW + (lane % LPR)*8

For every (BN, WGN, XTR) the host dispatches this checks that the map is a
bijection onto the tile, that every 16-byte access is aligned, that no two
waves' regions overlap, that the tiles fit the kernel's existing LDS
footprint, and what the bank rules of the LDS say about conflicts.
"""

import numpy as np
import pytest

WGM, BKP = 4, 40
# (BN, WGN, TC, XTR, smallest XR bucket): every pair geometry of the host
# dispatcher, SONATA_RB_GEOM variants included
GEOMS = [
    (32, 2, 2, 256, 272),
    (64, 2, 2, 128, 144),
    (128, 2, 3, 128, 144),
    (128, 2, 2, 64, 80),
    (256, 2, 1, 64, 80),
    (256, 2, 2, 128, 144),
]


def _consts(BN, WGN, XTR):
    WM, WN = XTR // WGM, BN // WGN
    CW = min(WN, 64)
    return dict(WM=WM, WN=WN, MT=WM // 16, NT=WN // 16, CW=CW, SP=CW + 4,
                NH=WN // CW, NTH=CW // 16, LPR=CW // 8, RPP=64 // (CW // 8),
                G=WM // (64 // (CW // 8)))


def _write_offsets(c, wave):
    """float offsets [lane, mi, rg, nj] of one column pass's writes."""
    lane = np.arange(64).reshape(64, 1, 1, 1)
    mi = np.arange(c["MT"]).reshape(1, -1, 1, 1)
    rg = np.arange(4).reshape(1, 1, 4, 1)
    nj = np.arange(c["NTH"]).reshape(1, 1, 1, -1)
    kl, il = lane >> 4, lane & 15
    row = mi * 16 + kl * 4 + rg
    col = nj * 16 + il
    return wave * c["WM"] * c["SP"] + row * c["SP"] + col, row, col


def _read_offsets(c, wave):
    """float offset of the first of 8 floats, [lane, g]; row; column."""
    lane = np.arange(64).reshape(64, 1)
    g = np.arange(c["G"]).reshape(1, -1)
    row = g * c["RPP"] + lane // c["LPR"]
    col = (lane % c["LPR"]) * 8 + 0 * g
    return wave * c["WM"] * c["SP"] + row * c["SP"] + col, row, col


@pytest.mark.parametrize("BN,WGN,TC,XTR,XR", GEOMS)
def test_map_is_a_bijection_onto_the_tile(BN, WGN, TC, XTR, XR):
    c = _consts(BN, WGN, XTR)
    assert c["NH"] * c["CW"] == c["WN"] and c["G"] * c["RPP"] == c["WM"]
    out = np.zeros((XTR, BN), dtype=np.int64)  # times each element is stored
    for wave in range(8):
        wr, wc = wave // WGN, wave % WGN
        for h in range(c["NH"]):
            lds = {}
            woff, wrow, wcol = _write_offsets(c, wave)
            # the value written is acc[mi][h*NTH + nj][rg]: tile element
            # (wr*WM + row, wc*WN + h*CW + col)
            vals = (wr * c["WM"] + wrow) * BN + wc * c["WN"] + h * c["CW"] + wcol
            woff, vals = np.broadcast_arrays(woff, vals)
            assert np.unique(woff).size == woff.size  # no two lanes collide
            lds = dict(zip(woff.ravel().tolist(), vals.ravel().tolist()))
            roff, rrow, rcol = _read_offsets(c, wave)
            for lane in range(64):
                for g in range(c["G"]):
                    m2 = wr * c["WM"] + int(rrow[lane, g])
                    col0 = wc * c["WN"] + h * c["CW"] + int(rcol[lane, g])
                    for q in range(8):
                        # what the lane reads is the element it stores
                        assert lds[int(roff[lane, g]) + q] == m2 * BN + col0 + q
                        out[m2, col0 + q] += 1
    assert (out == 1).all()


@pytest.mark.parametrize("BN,WGN,TC,XTR,XR", GEOMS)
def test_accesses_aligned_regions_disjoint_and_inside_lds(BN, WGN, TC, XTR, XR):
    c = _consts(BN, WGN, XTR)
    lds_bytes = (XR * BKP + XTR * (BN + 8) + TC * BN * BKP) * 2
    spans = []
    for wave in range(8):
        woff, _, _ = _write_offsets(c, wave)
        roff, _, rcol = _read_offsets(c, wave)
        assert (roff * 4 % 16 == 0).all()        # both ds_read_b128 of a lane
        assert ((roff + 4) * 4 % 16 == 0).all()
        assert (rcol % 8 == 0).all()             # 16-byte global groups
        lo = min(int(woff.min()), int(roff.min()))
        hi = max(int(woff.max()), int(roff.max()) + 7)
        assert lo == wave * c["WM"] * c["SP"]
        assert hi < (wave + 1) * c["WM"] * c["SP"]
        spans.append((lo, hi))
    for (_, hi), (lo, _) in zip(spans, spans[1:]):
        assert hi < lo
    assert (spans[-1][1] + 1) * 4 <= lds_bytes
    # GEMM 2's discarded rows (k <= 11) past Xt stay inside Ws behind it
    assert 10 * (BN + 8) * 2 <= TC * BN * BKP * 2


def _ways(banks, groups):
    """Worst number of distinct addresses on one bank within a lane group.
    banks: [lane, dwords] bank of every dword a lane touches."""
    worst = 1
    for grp in groups:
        seen = {}
        for lane in grp:
            for bk in banks[lane]:
                seen.setdefault(int(bk), set()).add(lane)
        worst = max(worst, max(len(v) for v in seen.values()))
    return worst


# ds_read_b128 serves four 16-lane groups; ds_write_b32 two 32-lane halves
B128_GROUPS = [
    [0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27],
    [4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31],
]
B128_GROUPS = B128_GROUPS + [[l + 32 for l in g] for g in B128_GROUPS]
B32_GROUPS = [list(range(32)), list(range(32, 64))]


@pytest.mark.parametrize("BN,WGN,TC,XTR,XR", GEOMS)
def test_lds_bank_spread(BN, WGN, TC, XTR, XR):
    """Writes (bank = dword mod 32 per 32-lane half) are conflict-free: the
    pitch CW + 4 puts rows 4 apart 16 banks apart.  The 16-byte reads (bank =
    dword mod 64 per 16-lane group) are at most 2-way: the groups of
    ds_read_b128 are not contiguous lanes, so with consecutive lanes on one
    row a group holds half rows of four different rows, and with rows one
    16-byte slot apart (pitch = 4 mod 64 dwords) two of its 16 lanes meet."""
    c = _consts(BN, WGN, XTR)
    woff, _, _ = _write_offsets(c, 0)
    for mi in range(c["MT"]):
        for rg in range(4):
            for nj in range(c["NTH"]):
                banks = (woff[:, mi, rg, nj] % 32).reshape(64, 1)
                assert _ways(banks, B32_GROUPS) == 1
    roff, _, _ = _read_offsets(c, 0)
    for g in range(c["G"]):
        for half in (0, 4):
            first = roff[:, g] + half
            banks = (first.reshape(64, 1) + np.arange(4)) % 64
            assert _ways(banks, B128_GROUPS) <= 2
