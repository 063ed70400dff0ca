"""The launch plan of the persistent fp16 GEMM (csrc/gemm_f16_p8.hip), host side: workgroups per XCD, tile rounds and strip height
asked of the very function the launcher calls (sampt_gemm_f16_p8_plan), and a restatement of the kernel's tile list under that
plan — every output tile belongs to exactly one workgroup, once.  Nothing here launches a kernel."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("sampt_gemm_f16_p8", "sampt_gemm_f16_p8_plan")
NT_M, NT_N, CAPS = range(1, 41), range(1, 21), range(1, 33)


@pytest.fixture(scope="module")
def lib():
    from sam_pt_amd import _lib
    return _lib.load()


def plan(lib, nt_m, nt_n, cap, trim, ragged=0):
    """(workgroups per XCD, rounds, strip rows) for nt_m x nt_n tiles; ragged: rows missing from the last 256-row panel"""
    w, r, s = C.c_int(-1), C.c_int(-1), C.c_int(-1)
    assert lib.sampt_gemm_f16_p8_plan(256 * nt_m - ragged, 256 * nt_n, cap, trim, C.byref(w), C.byref(r), C.byref(s)) == 0
    return w.value, r.value, s.value


def cdiv(a, b):
    return -(-a // b)


def decode(g, nt_m, nt_n, R):
    """The kernel's `decode`: strips of R row panels, column-major inside a strip, a short last strip of nt_m % R panels."""
    per_strip, nfull = R * nt_n, nt_m // R
    strip = g // per_strip
    if strip < nfull:
        t, rows = g - strip * per_strip, R
    else:
        strip, t, rows = nfull, g - nfull * per_strip, nt_m - nfull * R
    tn = t // rows
    return strip * R + (t - tn * rows), tn


def workgroup_lists(ntiles, nwg):
    """The kernel's tile list of workgroup (xcd, w): XCD x owns [ntiles * x >> 3, ntiles * (x + 1) >> 3), its workgroups step by nwg.
    A workgroup whose first index is past the end of its XCD's range returns at once (an empty list)."""
    return {(x, w): range((ntiles * x >> 3) + w, ntiles * (x + 1) >> 3, nwg) for x in range(8) for w in range(nwg)}


def test_plan_respects_the_cap_and_trimming_keeps_the_rounds(lib):
    for nt_m in NT_M:
        for nt_n in NT_N:
            tpx = cdiv(nt_m * nt_n, 8)                         # the largest share of an XCD
            for cap in CAPS:
                w0, r0, s0 = plan(lib, nt_m, nt_n, cap, 0)
                w1, r1, s1 = plan(lib, nt_m, nt_n, cap, 1)
                what = f"nt_m={nt_m} nt_n={nt_n} cap={cap}"
                assert 1 <= w1 <= w0 <= cap, what
                assert r0 == r1 == cdiv(tpx, w0) == cdiv(tpx, w1), what
                assert w0 == min(cap, tpx), what
                assert w1 == min(w for w in range(1, cap + 1) if cdiv(tpx, w) == r1), what
                assert s0 == s1 == min(4, nt_m), what
    # a ragged last panel counts as a panel; cap 0 = one workgroup per CU
    assert plan(lib, 5, 5, 2, 1, ragged=255) == plan(lib, 5, 5, 2, 1)
    assert plan(lib, 12, 20, 0, 0) == plan(lib, 12, 20, 32, 0) == (30, 1, 4)
    assert plan(lib, 40, 20, 0, 0) == (32, 4, 4) and plan(lib, 40, 20, 0, 1) == (25, 4, 4)


def test_every_tile_runs_exactly_once_under_every_plan(lib):
    decoded = {}
    for nt_m in NT_M:
        for nt_n in NT_N:
            R = min(4, nt_m)
            tiles = [decode(g, nt_m, nt_n, R) for g in range(nt_m * nt_n)]
            assert sorted(tiles) == [(tm, tn) for tm in range(nt_m) for tn in range(nt_n)], f"decode is no bijection at {nt_m} x {nt_n}"
            decoded[nt_m, nt_n] = tiles
    checked = {}
    for nt_m in NT_M:
        for nt_n in NT_N:
            ntiles = nt_m * nt_n
            for cap in CAPS:
                for trim in (0, 1):
                    nwg, rounds, R = plan(lib, nt_m, nt_n, cap, trim)
                    assert R == min(4, nt_m)
                    if (ntiles, nwg) not in checked:
                        lists = workgroup_lists(ntiles, nwg)
                        seen = sorted(g for r in lists.values() for g in r)
                        assert seen == list(range(ntiles)), f"{ntiles} tiles on {nwg} workgroups per XCD: a tile is missed or run twice"
                        checked[ntiles, nwg] = max(len(r) for r in lists.values())
                    assert checked[ntiles, nwg] <= rounds, f"nt_m={nt_m} nt_n={nt_n} cap={cap} trim={trim}: a tile list longer than rounds"
    # ... and through decode, for the two shapes of the GPU test and a capped ViT-B launch
    for nt_m, nt_n, cap in ((10, 3, 1), (5, 5, 2), (5, 5, 3), (16, 12, 7)):
        nwg, rounds, R = plan(lib, nt_m, nt_n, cap, 1)
        owners = {}
        for key, r in workgroup_lists(nt_m * nt_n, nwg).items():
            for g in r:
                owners.setdefault(decoded[nt_m, nt_n][g], []).append(key)
        assert len(owners) == nt_m * nt_n and all(len(v) == 1 for v in owners.values())


def test_plan_gives_the_vit_h_figures(lib):
    """ViT-H, 8 frames, proj / fc2 (N = 1280): 128 x 5 tiles = 80 per XCD, 3 rounds on 30 workgroups and on 27."""
    assert plan(lib, 128, 5, 30, 0) == (30, 3, 4)
    assert plan(lib, 128, 5, 30, 1) == (27, 3, 4)
    assert plan(lib, 128, 5, 0, 1) == (27, 3, 4)
    assert plan(lib, 128, 5, 26, 1)[1] == 4


def test_plan_follows_the_process_setting_when_asked(lib):
    try:
        assert lib.sampt_gemm_set_trim(0) == 0
        assert plan(lib, 128, 5, 30, -1) == (30, 3, 4)
        assert plan(lib, 128, 5, 30, 1) == (27, 3, 4)
    finally:
        assert lib.sampt_gemm_set_trim(1) == 0
    assert plan(lib, 128, 5, 30, -1) == (27, 3, 4)
    assert plan(lib, 128, 5, 30, 0) == (30, 3, 4)


def test_plan_and_strict_entry_refuse_bad_arguments(lib):
    w, r, s = C.c_int(-9), C.c_int(-9), C.c_int(-9)
    refs = (C.byref(w), C.byref(r), C.byref(s))
    assert lib.sampt_gemm_f16_p8_plan(255, 256, 0, 1, *refs) == -1          # fewer rows than the kernel takes
    assert lib.sampt_gemm_f16_p8_plan(256, 0, 0, 1, *refs) == -1
    assert lib.sampt_gemm_f16_p8_plan(256, 384, 0, 1, *refs) == -1          # N % 256
    assert lib.sampt_gemm_f16_p8_plan(256, 256, 33, 1, *refs) == -1
    assert lib.sampt_gemm_f16_p8_plan(256, 256, -1, 1, *refs) == -1
    assert lib.sampt_gemm_f16_p8_plan(256, 256, 0, 2, *refs) == -1
    assert lib.sampt_gemm_f16_p8_plan(256, 256, 0, -2, *refs) == -1
    assert lib.sampt_gemm_f16_p8_plan(256, 256, 0, 1, None, C.byref(r), C.byref(s)) == -1
    assert lib.sampt_gemm_f16_p8_plan(256, 256, 0, 1, C.byref(w), None, C.byref(s)) == -1
    assert lib.sampt_gemm_f16_p8_plan(256, 256, 0, 1, C.byref(w), C.byref(r), None) == -1
    assert (w.value, r.value, s.value) == (-9, -9, -9), "a refused query wrote its outputs"
    # the strict entry checks its arguments before it looks at a pointer's target (these are never dereferenced on the host)
    p = 4096
    call = lambda dtype=1, A=p, heads=0, hd=0, rows=0, wgs=0, stagger=0: lib.sampt_gemm_f16_p8(
        dtype, A, p, None, None, p, 512, 256, 128, 0, 1.0, None, None, 0, 0, heads, hd, rows, wgs, stagger, None)
    assert call(dtype=0) == -1 and call(dtype=5) == -1
    assert call(A=None) == -1
    assert call(wgs=33) == -1 and call(wgs=-1) == -1
    assert call(stagger=9) == -1
    assert call(dtype=2, heads=2, hd=0, rows=512) == -1                       # half a head-major triple
    assert call(dtype=2, heads=2, hd=6, rows=512) == -1                       # hd % 4
    assert call(dtype=2, heads=3, hd=64, rows=512) == -1                      # N % (heads * hd)
    assert call(dtype=2, heads=2, hd=64, rows=100) == -1                      # fewer destination rows than M, no rowmap


def test_c_abi_declares_binds_and_exports_the_p8_entry_points(lib):
    from sam_pt_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "sampt_hip.h")).read()
    declared = set(re.findall(r"\b(sampt_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW_SYMBOLS:
        assert name in declared, f"{name} is not declared in include/sampt_hip.h"
        assert name in _lib._SIGS, f"{name} has no ctypes signature in _lib._SIGS"
        assert hasattr(lib, name), f"{name} is not exported by libsampt_hip.so"
        assert _lib._SIGS[name][0] is _lib.c_int
    assert _lib._SIGS["sampt_gemm_f16_p8"][1][-1] is _lib._P                  # house style: stream last
    proto = re.search(r"int sampt_gemm_f16_p8\((.*?)\);", hdr, re.S).group(1)
    assert len(proto.split(",")) == len(_lib._SIGS["sampt_gemm_f16_p8"][1]) == 21
    assert "sampt_gemm_f16_p8_plan" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
