"""Batch-invariant mask decoding, host side: the routing of the decoder's f32 GEMMs and the key split of its token -> image
attention, asked of the very functions the dispatchers call (sampt_gemm_f32_route, sampt_attn_t2i_plan), and the
``SamHip(batch_invariant_decode=...)`` switch.  Nothing here launches a kernel."""
import ctypes as C

import pytest

# every (N, K) of a plain f32 product the decoder issues ("Batch-invariant decoding")
DEC_N = (256, 128, 2048, 32, 4, 3, 1)
DEC_K = (256, 128, 2048)
ROWS = (1, 4, 10, 16, 17, 30, 170, 192, 193, 240, 2560)
FRAMES = (1, 2, 3, 16, 17, 128)
T2I_REC = 144                      # floats of one partial softmax state (include/sampt_hip.h, sampt_attn_t2i_plan)
INV_ROUTES = (3, 4)                # row-invariant thin / one wave per element


@pytest.fixture(scope="module")
def lib():
    from sam_pt_amd import _lib
    return _lib.load()


def route(lib, M, N, K, invariant, lda=0, ldc=0):
    r, kp = C.c_int(-1), C.c_int(-1)
    assert lib.sampt_gemm_f32_route(M, N, K, lda, ldc, invariant, C.byref(r), C.byref(kp)) == 0
    return r.value, kp.value


def plan(lib, F, Nq, Nk, invariant):
    ks, kper = C.c_int(-1), C.c_int(-1)
    assert lib.sampt_attn_t2i_plan(F, Nq, Nk, invariant, C.byref(ks), C.byref(kper)) == 0
    return ks.value, kper.value


@pytest.mark.parametrize("K", DEC_K)
@pytest.mark.parametrize("N", DEC_N)
def test_invariant_gemm_route_ignores_rows(lib, N, K):
    got = {route(lib, M, N, K, 1) for M in ROWS}
    assert len(got) == 1, f"N={N} K={K}: the row-invariant route depends on M: {sorted(got)}"
    r, kparts = next(iter(got))
    assert r in INV_ROUTES and kparts >= 1
    # strided token rows (lda = Nt * C, the heads' first layers) and a wider C (ldc = 3 * N, decode_points' hypernetwork block)
    for Nt in (7, 21):
        assert {route(lib, M, N, K, 1, lda=Nt * 256) for M in ROWS} == got
    assert len({route(lib, M, N, K, 1, ldc=3 * N) for M in ROWS}) == 1


def test_invariant_gemm_route_is_a_function_of_k(lib):
    """The thin route's K shares follow K alone — the same for every N it serves."""
    for K in DEC_K:
        assert len({route(lib, 40, N, K, 1) for N in (256, 128, 2048, 32, 4)}) == 1
    assert route(lib, 40, 1, 256, 1)[0] == 4 and route(lib, 40, 3, 256, 1)[0] == 4      # N % 4 != 0: one wave per element
    assert route(lib, 40, 4, 256, 1, ldc=3)[0] == 4                                      # ldc % 4 != 0 likewise


def test_default_gemm_route_depends_on_rows(lib):
    """The routes this mode replaces: they change with M at the shapes ISSUE / DESIGN name, so the test above can tell."""
    assert route(lib, 16, 256, 256, 0)[0] == 0 and route(lib, 17, 256, 256, 0)[0] == 1          # skinny -> thin at F * Nt = 17
    assert route(lib, 16, 1, 256, 0)[0] == 0 and route(lib, 17, 1, 256, 0)[0] == 2              # IoU head, N = 1: skinny -> tiled
    assert route(lib, 192, 2048, 256, 0)[0] == 1 and route(lib, 193, 2048, 256, 0)[0] == 2      # thin -> tiled at 128 tiles
    # split-K of the tiled kernel follows the tile count (N = 1 is refused by the thin kernel: tiled from 17 rows on)
    ks = {route(lib, M, 1, 2048, 0) for M in (17, 2560)}
    assert all(r == 2 for r, _ in ks) and len(ks) > 1, ks
    for N in DEC_N:
        for K in DEC_K:
            assert all(route(lib, M, N, K, 0)[0] not in INV_ROUTES for M in ROWS)
    assert len({route(lib, M, N, K, 0) for M in ROWS for N in DEC_N for K in DEC_K}) > 3


@pytest.mark.parametrize("Nk", (4096, 1024))
def test_invariant_t2i_plan_ignores_batch(lib, Nk):
    from sam_pt_amd import _lib
    got = {plan(lib, F, Nq, Nk, 1) for F in FRAMES for Nq in range(7, 22)}
    assert len(got) == 1, f"Nk={Nk}: the fixed key split depends on F or Nq: {sorted(got)}"
    KS, kper = next(iter(got))
    assert got == {plan(lib, 1, Nq, Nk, 0) for Nq in range(7, 22)}, "the fixed split is the default's plan for one item"
    assert KS * kper >= Nk and (KS - 1) * kper < Nk and kper % 32 == 0 and kper >= 64
    # decode_points' shared first layer: one item with n * Nt queries
    assert plan(lib, 1, 128 * 21, Nk, 1) == (KS, kper)
    for F in FRAMES:
        for Nq in (7, 8, 9, 21):
            need = F * Nq * KS * T2I_REC * 4
            assert _lib.workspace_bytes("sampt_attention_t2i_workspace_bytes", F, Nq, Nk) >= need
            ks0, _ = plan(lib, F, Nq, Nk, 0)
            assert _lib.workspace_bytes("sampt_attention_t2i_workspace_bytes", F, Nq, Nk) >= F * Nq * ks0 * T2I_REC * 4
    assert _lib.workspace_bytes("sampt_attention_t2i_workspace_bytes", 1, 128 * 21, Nk) >= 128 * 21 * KS * T2I_REC * 4


def test_default_t2i_plan_depends_on_batch(lib):
    assert len({plan(lib, F, 13, 4096, 0) for F in FRAMES}) > 1
    assert len({plan(lib, F, 13, 1024, 0) for F in FRAMES}) > 1
    assert plan(lib, 128, 13, 4096, 0)[0] < plan(lib, 1, 13, 4096, 0)[0]


def test_route_queries_reject_bad_arguments(lib):
    r, kp = C.c_int(), C.c_int()
    assert lib.sampt_gemm_f32_route(0, 4, 256, 0, 0, 1, C.byref(r), C.byref(kp)) != 0
    assert lib.sampt_gemm_f32_route(4, 4, 255, 0, 0, 1, C.byref(r), C.byref(kp)) != 0
    assert lib.sampt_gemm_f32_route(4, 4, 256, 0, 0, 2, C.byref(r), C.byref(kp)) != 0
    assert lib.sampt_attn_t2i_plan(1, 0, 4096, 1, C.byref(r), C.byref(kp)) != 0
    assert lib.sampt_dec_set_batch_invariant(None, 1) != 0


def test_samhip_option_sets_the_clip_chain_length():
    from sam_pt_amd.sam_predictor import SamHip
    on = SamHip(variant="vit_t", batch_invariant_decode=True)
    assert on.batch_invariant_decode is True and on.clip_decode_batch == on.max_decode_batch == 128
    off = SamHip(variant="vit_t")
    assert off.batch_invariant_decode is False and off.clip_decode_batch == 1
    assert SamHip(variant="vit_t", batch_invariant_decode=True, clip_decode_batch=4).clip_decode_batch == 4
    assert SamHip(variant="vit_t", batch_invariant_decode=True, max_decode_batch=32).clip_decode_batch == 32
    # ViT predictors: None keeps meaning "chunk by max_decode_batch" in either mode
    assert SamHip(variant="vit_b", batch_invariant_decode=True).clip_decode_batch is None
    assert SamHip(variant="vit_b").clip_decode_batch is None
