"""What the prompt-assembly tests share (tests/test_prompt_assembly_cpu.py, tests/test_gpu_prompt_assembly.py): the seeded cases and
the yardstick — ``SamPt._prepare_points`` followed by ``ResizeLongestSide.apply_coords`` item by item, packed the way
``SamPt._enqueue_sam_fused`` packs its host block."""
import functools
from types import SimpleNamespace

import numpy as np

from sam_pt_amd.sam_predictor import ResizeLongestSide
from sam_pt_amd.sam_pt import PointVisibilityType, SamPt

T = 3
SIZE = (480, 854)                 # (height, width) -> 576 x 1024: an anisotropic pair of factors (1024 / 854, 576 / 480)
CODES = [float(c.value) for c in PointVisibilityType]          # 1, 0, -1, -2, -3, -4

# M: 1 (no other objects), 2, 9 / 10 (with pp = 8 the others contribute up to 64 / 72 points: one wave exactly, one more), 70 (a
# candidate list longer than one workgroup's round).  (pp, P): one negative point, none (P == pp), a short object.
CASES = [(M, pp, P, negatives, add_others) for M in (1, 2, 9, 10, 70) for pp, P in ((8, 9), (16, 16), (3, 5))
         for negatives in (False, True) for add_others in (True, False)]


def scales():
    new_h, new_w = ResizeLongestSide(1024).get_preprocess_shape(SIZE[0], SIZE[1], 1024)
    return new_w / SIZE[1], new_h / SIZE[0]


def make_tracks(M, pp, P, seed=0):
    """traj (T,M,P,2) float32 inside the frame, vis (T,M,P) float32 codes: frame 0 random codes, with every code of
    PointVisibilityType on object 0 and an object whose leading points are all invisible (an empty segment); frame 1 nothing visible
    (k = 0 everywhere); frame 2 random, object 0 with only its tail visible (npos = 0 with negatives, k = 0 of its own when P == pp)."""
    rng = np.random.default_rng(1000 * M + 10 * pp + P + seed)
    traj = (rng.random((T, M, P, 2)) * np.array([SIZE[1], SIZE[0]])).astype(np.float32)
    vis = rng.choice(np.array(CODES + [1.0, 1.0, 1.0], dtype=np.float32), size=(T, M, P))
    n = min(P, len(CODES))
    vis[0, 0, :n] = CODES[:n]
    vis[0, M - 1, :min(pp, P)] = [0.0, -2.0, -3.0, -4.0, -1.0][M % 5]
    vis[1] = rng.choice(np.array(CODES[1:], dtype=np.float32), size=(M, P))
    vis[2, 0, :pp] = 0.0
    vis[2, 0, pp:] = 1.0
    return traj, vis


@functools.lru_cache(maxsize=None)
def reference(M, pp, P, negatives, add_others):
    """-> (traj, vis, xy (T*M,kmax,2) f32, lab (T*M,kmax) i32, k (T*M,) i32, npos (T*M,) i32) by the host loop; treat as read-only."""
    traj, vis = make_tracks(M, pp, P)
    me = SimpleNamespace(positive_points_per_mask=pp, negative_points_per_mask=1 if negatives else 0,
                         add_other_objects_positive_points_as_negative_points=add_others, max_other_objects_positive_points=None)
    tf = ResizeLongestSide(1024)
    vis_b = vis == 1
    prompts = []
    for t in range(T):
        for m in range(M):
            c, l = SamPt._prepare_points(me, traj, vis_b, t, m, M)
            if len(c):
                c = tf.apply_coords(c, SIZE)
            prompts.append((c, l))
    kmax = max(1, max(len(c) for c, _ in prompts))
    xy = np.zeros((len(prompts), kmax, 2), dtype=np.float32)
    lab = np.zeros((len(prompts), kmax), dtype=np.int32)
    for i, (c, l) in enumerate(prompts):
        xy[i, :len(c)] = c
        lab[i, :len(c)] = l
    k = np.array([len(c) for c, _ in prompts], dtype=np.int32)
    npos = np.array([int((l == 1).sum()) for _, l in prompts], dtype=np.int32)
    for a in (traj, vis, xy, lab, k, npos):
        a.setflags(write=False)
    return traj, vis, xy, lab, k, npos
