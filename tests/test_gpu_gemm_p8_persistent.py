"""The persistent fp16 GEMM (csrc/gemm_f16_p8.hip) with SEVERAL output tiles per workgroup: small matrices under a workgroup cap,
so that every launch walks a tile list — the stage cursor crosses tile boundaries, the gather offsets, the accumulators and the
epilogue's per-tile terms are refreshed, XCDs hold different numbers of tiles and the last strip is short.  All launches go
through sampt_gemm_f16_p8, which runs on that kernel or fails (no other kernel can answer for it), and every case first asks
sampt_gemm_f16_p8_plan how many rounds its launch has.  Against an fp64 product with the epilogue applied in fp64, and bit for
bit against the launch of the same call that gives every workgroup one tile."""
import contextlib
import ctypes as C
import functools

import pytest
import torch
import torch.nn.functional as F

from tests.util import rel_err

pytestmark = pytest.mark.gpu

SHAPES = [(2400, 768),      # 10 row panels: strips of 4, 4, 2; 30 tiles, 3 or 4 per XCD; ragged last panel (96 rows)
          (1200, 1280)]     # 5 row panels: strips of 4, 1; 25 tiles; ragged last panel (176 rows)
KERNEL_K = [128, 384]       # K of the kernel (x3: twice the logical K); 128 = two K-tiles: the stage cursor changes tile in every pass
CAPS = [1, 2, 3, 0]         # workgroups per XCD; 0 = one per CU, here one per tile.  The largest share of an XCD is 4 tiles on both
                            # shapes, so the trim rule would turn cap 3 into the grid of cap 2: cap 3 runs untrimmed (launch_trim) —
                            # three workgroups per XCD with tile lists of 2, 1, 1 (or 1, 1, 1 where the XCD holds 3 tiles)
MOD = 100                   # rows of the broadcast residual (res_mod)
GUARD = 5                   # rows of C beyond the last destination row
# name: (dtype of sampt_gemm_ex, act, head-major)
VARIANTS = {"f16_f32": (1, 0, False), "f16_f16": (2, 0, False), "f16_gelu_f32": (1, 2, False), "f16_gelu_f16": (2, 2, False),
            "f16_head_major": (2, 0, True), "x3_f32": (3, 0, False), "x3_x3rows": (4, 0, False), "x3_gelu_x3rows": (4, 2, False)}
HEADS = {768: (4, 64), 1280: (4, 80)}       # N: (heads, hd) — 80-column heads straddle the 256-column tiles


@pytest.fixture(scope="module")
def lib():
    from sam_pt_amd import _lib
    return _lib.load()


def P(t):
    from sam_pt_amd import _lib
    return _lib.ptr(t)


def S():
    from sam_pt_amd import _lib
    return _lib.stream_ptr()


def ok(rc, what=""):
    from sam_pt_amd import _lib
    _lib.check(rc, what)


def plan(lib, M, N, cap, trim=-1):
    """(workgroups per XCD, rounds, strip rows) of the launch; trim -1: under the process's setting"""
    w, r, s = C.c_int(-1), C.c_int(-1), C.c_int(-1)
    ok(lib.sampt_gemm_f16_p8_plan(M, N, cap, trim, C.byref(w), C.byref(r), C.byref(s)), "p8 plan")
    return w.value, r.value, s.value


@contextlib.contextmanager
def launch_trim(lib, cap):
    """sampt_gemm_set_trim(0) around the launches of cap 3 (see CAPS); the default everywhere else"""
    try:
        if cap == 3:
            ok(lib.sampt_gemm_set_trim(0), "set_trim")
        yield
    finally:
        ok(lib.sampt_gemm_set_trim(1), "set_trim")


def require_rounds(lib, M, N, cap):
    """What a case needs to mean anything: the reference launch has one tile per workgroup, the capped one several, and the XCDs'
    shares differ."""
    ntiles = ((M + 255) // 256) * (N // 256)
    shares = {(ntiles * (x + 1) >> 3) - (ntiles * x >> 3) for x in range(8)}
    assert len(shares) > 1, f"{M} x {N}: every XCD holds {shares} tiles"
    assert plan(lib, M, N, 0)[1] == 1, "the reference launch must give every workgroup one tile"
    wgs, rounds, strip = plan(lib, M, N, cap)
    assert strip == 4 and ((M + 255) // 256) % 4 != 0, "no short last strip"
    if cap == 1:
        assert wgs == 1 and rounds >= 3
    elif cap in (2, 3):
        assert wgs == cap and rounds >= 2
    return rounds


@functools.lru_cache(maxsize=None)
def problem(M, N, kk, x3):
    """Operands, row maps, residuals and the fp64 product of one shape (computed once, read-only afterwards).  The reference
    multiplies the very values the kernel is given: the fp16 operands, or the f32 ones the x3 rows are split from."""
    from sam_pt_amd.pack import F16X3_WSHIFT, x3_rows
    K = kk // 2 if x3 else kk
    g = torch.Generator().manual_seed(M * 3 + N + kk + (1 if x3 else 0))
    A = torch.randn(M, K, generator=g)
    W = torch.randn(N, K, generator=g) / K ** 0.5
    b = torch.randn(N, generator=g)
    D = M + 3                                                      # destination rows: a permutation with holes and 7 dropped rows
    dest = torch.randperm(D, generator=g)[:M].to(torch.int32)
    dest[torch.randperm(M, generator=g)[:7]] = -1
    src = torch.randperm(M, generator=g).to(torch.int32)
    if not x3:
        A, W = A.half(), W.half()
    acc = A[src.long()].double() @ W.double().t() + b.double()
    keep = dest >= 0
    written = dest[keep].long()
    untouched = torch.ones(D + GUARD, dtype=torch.bool)
    untouched[written] = False
    dev = torch.device("cuda:0")
    p = dict(M=M, N=N, K=K, rows=D + GUARD, acc={0: acc, 2: F.gelu(acc)}, keep=keep, written=written, untouched=untouched,
             res=torch.randn(D + GUARD, N, generator=g), res_mod=torch.randn(MOD, N, generator=g),
             b=b.to(dev), dest=dest.to(dev), src=src.to(dev))
    p["A"] = (x3_rows(A) if x3 else A).to(dev)
    p["W"] = (x3_rows(W, F16X3_WSHIFT) if x3 else W).to(dev)
    p["res_mod_dev"] = p["res_mod"].to(dev)
    if x3:
        p["A32"], p["W32"], p["e32"] = A[src.long()].contiguous().to(dev), W.to(dev), {}
    return p


def expected(p, act, mode):
    """fp64: 7.0 everywhere, act(A[src] . W^T + bias) + residual at the destination rows"""
    ref = torch.full((p["rows"], p["N"]), 7.0, dtype=torch.float64)
    w = p["written"]
    r = p["res"][w] if mode == "inplace" else p["res_mod"][w % MOD]
    ref[w] = p["acc"][act][p["keep"]] + r.double()
    return ref


def prefill(p, variant, mode):
    """C before the launch: 7.0, and for the in-place residual (res == C, the encoder's proj / fc2) the residual at the rows the launch
    writes"""
    from sam_pt_amd.pack import x3_rows
    dtype, _, hm = VARIANTS[variant]
    rows, N = p["rows"], p["N"]
    if dtype == 4:
        return x3_rows(torch.full((rows, N), 7.0)).to(p["b"].device)
    c = torch.full((rows, N), 7.0, dtype=torch.float16 if dtype == 2 else torch.float32)
    if mode == "inplace":
        c[p["written"]] = p["res"][p["written"]]
    if hm:
        heads, hd = HEADS[N]
        c = c.view(N // (heads * hd), heads, rows, hd).clone()     # (all 7.0: the shape alone matters)
    return c.to(p["b"].device)


def launch(lib, p, variant, mode, cap, stagger=0, c0=None):
    dtype, act, hm = VARIANTS[variant]
    Cd = (prefill(p, variant, mode) if c0 is None else c0).clone()
    heads, hd = HEADS[p["N"]] if hm else (0, 0)
    res, mod = (Cd, 0) if mode == "inplace" else (p["res_mod_dev"], MOD)
    alpha = 2.0 ** -8 if dtype >= 3 else 1.0
    rc = lib.sampt_gemm_f16_p8(dtype, P(p["A"]), P(p["W"]), P(p["b"]), P(res), P(Cd), p["M"], p["N"], p["K"], act, alpha, P(p["dest"]),
                               P(p["src"]), mod, 0, heads, hd, p["rows"] if hm else 0, cap, stagger, S())
    ok(rc, f"sampt_gemm_f16_p8 {variant} cap {cap}")
    return Cd


def token_rows(Cd, variant):
    """the output as f32 [rows][N] on the host"""
    from sam_pt_amd.pack import x3_unrows
    dtype, _, hm = VARIANTS[variant]
    if dtype == 4:
        return x3_unrows(Cd.cpu())
    if hm:
        return Cd.permute(2, 0, 1, 3).reshape(Cd.shape[2], -1).float().cpu()
    return Cd.float().cpu()


def untouched_rows(Cd, p, variant):
    """the stored bits of the rows no GEMM row maps to, guard rows included"""
    u = p["untouched"].to(Cd.device)
    return Cd[:, :, u] if VARIANTS[variant][2] else Cd[u]


def bar(lib, p, variant):
    """fp16 output: 2e-3; fp16 in / f32 out: 2e-5 sqrt(K); x3: twice the error of the exact f32 GEMM on the same operands, at least 2e-6"""
    dtype, act, _ = VARIANTS[variant]
    if dtype == 2:
        return 2e-3
    if dtype == 1:
        return 2e-5 * p["K"] ** 0.5
    if act not in p["e32"]:
        C32 = torch.empty(p["M"], p["N"], device=p["b"].device)
        ok(lib.sampt_gemm(0, P(p["A32"]), P(p["W32"]), P(p["b"]), None, P(C32), p["M"], p["N"], p["K"], act, 1.0, S()), "gemm f32")
        p["e32"][act] = rel_err(C32, p["acc"][act])
    return max(2e-6, 2.0 * p["e32"][act])


def modes(variant):
    """every variant: bias + rowmap (dropped rows) + a_rowmap + broadcast residual; f32 output also with the residual in place"""
    return ("mod", "inplace") if VARIANTS[variant][0] in (1, 3) else ("mod",)


@pytest.mark.parametrize("kk", KERNEL_K)
@pytest.mark.parametrize("M,N", SHAPES)
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_tile_lists_against_fp64(lib, dev, variant, M, N, kk):
    p = problem(M, N, kk, VARIANTS[variant][0] >= 3)
    tol = bar(lib, p, variant)
    for mode in modes(variant):
        ref = expected(p, VARIANTS[variant][1], mode)
        c0 = prefill(p, variant, mode)
        one_tile = None
        for cap in reversed(CAPS):                                 # the one-tile-per-workgroup launch first
            with launch_trim(lib, cap):
                rounds = require_rounds(lib, M, N, cap)
                Cd = launch(lib, p, variant, mode, cap, c0=c0)
            torch.cuda.synchronize()
            got = token_rows(Cd, variant)
            w = p["written"]
            err = rel_err(got[w], ref[w])
            print(f"{variant} {M}x{N}x{kk} {mode} cap {cap}: {rounds} rounds, rel err {err:.3g} (bar {tol:.3g})")
            assert err < tol, f"{mode}, cap {cap} ({rounds} rounds): {err} >= {tol}"
            assert torch.equal(untouched_rows(Cd, p, variant), untouched_rows(c0, p, variant)) and bool((got[p["untouched"]] == 7.0).all()), \
                f"{mode}, cap {cap}: rows outside the row map or guard rows were written"
            if cap == 0:
                one_tile = Cd
            else:
                assert torch.equal(Cd, one_tile), f"{mode}, cap {cap}: {rounds} rounds differ from one tile per workgroup"


@pytest.mark.parametrize("kk", KERNEL_K)
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_plan_schedule_and_phase_groups_leave_the_bits_alone(lib, dev, variant, kk):
    """The header's promises for sampt_gemm_set_trim, sampt_gemm_set_schedule, the phase groups and the workgroup caps."""
    M, N = SHAPES[0]
    p = problem(M, N, kk, VARIANTS[variant][0] >= 3)
    require_rounds(lib, M, N, 1)
    for mode in modes(variant):
        c0 = prefill(p, variant, mode)
        one_tile = launch(lib, p, variant, mode, 0, stagger=1, c0=c0)
        w = p["written"]                                           # (the product ran: every destination row lost its prefill)
        assert bool((token_rows(one_tile, variant)[w] != token_rows(c0, variant)[w]).any(dim=1).all())
        try:
            for trim in (0, 1):
                ok(lib.sampt_gemm_set_trim(trim), "set_trim")
                for sched in (0, 1):
                    ok(lib.sampt_gemm_set_schedule(sched), "set_schedule")
                    for groups, per_call in ((1, True), (2, True), (3, True), (2, False), (3, False)):
                        ok(lib.sampt_gemm_set_stagger(0 if per_call else groups), "set_stagger")
                        for cap in (1, 2, 3, 5, 32):
                            Cd = launch(lib, p, variant, mode, cap, stagger=groups if per_call else 0, c0=c0)
                            assert torch.equal(Cd, one_tile), \
                                f"{mode}: cap {cap}, trim {trim}, schedule {sched}, {groups} phase groups ({'call' if per_call else 'process'})"
        finally:
            ok(lib.sampt_gemm_set_trim(1), "set_trim")
            ok(lib.sampt_gemm_set_schedule(0), "set_schedule")
            ok(lib.sampt_gemm_set_stagger(0), "set_stagger")


@pytest.mark.parametrize("kk", KERNEL_K)
@pytest.mark.parametrize("M,N", SHAPES)
def test_head_major_bits_equal_token_major_bits(lib, dev, M, N, kk):
    """Element for element the bits of the dtype-2 launch at the permuted address, with a row map — 3 or 4 tiles per workgroup at cap 1,
    1 or 2 at caps 2 and 3."""
    p = problem(M, N, kk, False)
    heads, hd = HEADS[N]
    for cap in (1, 2, 3):
        with launch_trim(lib, cap):
            require_rounds(lib, M, N, cap)
            tm = launch(lib, p, "f16_f16", "mod", cap)
            hm = launch(lib, p, "f16_head_major", "mod", cap)
        assert bool((tm[p["written"].to(dev)] != 7.0).all(dim=1).any())     # (the product ran: 7.0 is the prefill)
        assert torch.equal(hm, tm.reshape(p["rows"], -1, heads, hd).permute(1, 2, 0, 3).contiguous()), f"cap {cap}"


def test_strict_entry_refuses_what_the_kernel_does_not_take(lib, dev):
    """-3 (SAMPT_ERR_UNSUPPORTED), never another kernel: C keeps its bits."""
    g = torch.Generator().manual_seed(5)
    buf = torch.randn(512 * 256 + 8, generator=g).half().to(dev)
    A, A_off = buf[:512 * 256], buf[4:4 + 512 * 256]              # the second starts 8 bytes into the allocation
    W = torch.randn(512 * 256, generator=g).half().to(dev)
    Cd = torch.full((512 * 512,), 7.0, device=dev)

    def call(dtype, A_, M, N, K, hm=(0, 0, 0)):
        return lib.sampt_gemm_f16_p8(dtype, P(A_), P(W), None, None, P(Cd), M, N, K, 0, 1.0, None, None, 0, 0, *hm, 0, 0, S())

    assert call(1, A, 255, 256, 128) == -3                         # M < 256
    assert call(1, A, 256, 384, 128) == -3                         # N % 256
    assert call(1, A, 256, 256, 192) == -3                         # K % 128
    assert call(3, A, 256, 256, 96) == -3                          # x3: the stored K (2 x 96) % 128
    assert call(1, A_off, 256, 256, 128) == -3                     # A not 16-byte aligned
    assert call(3, A, 512, 256, 64, hm=(2, 64, 512)) == -3         # x3 product with fp16 (head-major) output
    assert call(4, A, 512, 256, 64, hm=(2, 64, 512)) == -3
    torch.cuda.synchronize()
    assert bool((Cd == 7.0).all()), "a refused call wrote to C"
    ok(call(1, A, 256, 256, 128), "the same call, supported")      # (and the aligned, supported twin runs)
    torch.cuda.synchronize()
    assert not bool((Cd[:256 * 256] == 7.0).any()) and bool((Cd[256 * 256:] == 7.0).all())


@pytest.mark.parametrize("precision", ["f16", "f16x3"])
def test_vit_b_embeddings_do_not_depend_on_the_workgroup_plan(lib, dev, precision):
    """ViT-B on two landscape frames (the compact live-row stream: real rowmap / a_rowmap in the windowed blocks, the residual in place
    in proj / fc2): the embeddings under workgroup caps, per-kind caps and without trimming are the bits of the default launch."""
    from sam_pt_amd.sam_predictor import SamHip, SamPredictor
    hw = (576, 1024)
    g = torch.Generator().manual_seed(21)
    frames = torch.randint(0, 256, (2, 3) + hw, generator=g, dtype=torch.uint8).to(dev)
    # at least the live tokens reach every GEMM (2 frames x 36 x 64): qkv / proj / fc1 / fc2 have N = 2304 / 768 / 3072 / 768
    live = 2 * (hw[0] // 16) * 64
    assert plan(lib, live, 2304, 7)[1] >= 2 and plan(lib, live, 3072, 7)[1] >= 2
    assert all(plan(lib, live, n, cap)[1] >= 2 for n, cap in zip((2304, 768, 3072, 768), (5, 3, 6, 2)))
    # one workgroup per CU runs every launch of this size in one round, where trimming has nothing to do: also try it under a cap of 20
    assert all(plan(lib, m, 2304, 20, 1)[0] < plan(lib, m, 2304, 20, 0)[0] == 20 for m in (live, 2 * 4096))
    pred = SamPredictor(SamHip("vit_b", precision=precision, seed=72, max_batch=2).to(dev))
    base = pred.encode_frames(frames).clone()
    assert pred._dead_cache[hw] is not None, "the compact live-row stream was not taken"
    assert bool(torch.isfinite(base).all()) and float(base.abs().max()) > 0
    try:
        for wgs in (0, 7, (5, 3, 6, 2)):
            pred.set_gemm_workgroups(wgs)
            assert torch.equal(pred.encode_frames(frames), base), f"set_gemm_workgroups({wgs})"
        ok(lib.sampt_gemm_set_trim(0), "set_trim")
        for wgs in (0, 20):
            pred.set_gemm_workgroups(wgs)
            assert torch.equal(pred.encode_frames(frames), base), f"sampt_gemm_set_trim(0), set_gemm_workgroups({wgs})"
    finally:
        ok(lib.sampt_gemm_set_trim(1), "set_trim")
        pred.set_gemm_workgroups(0)
