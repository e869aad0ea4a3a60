"""Trimmed-ICP refinement of one MCTS child state restated in numpy, from the header of csrc/tricp_states.hip and the
comment of pgp_tricp_states in include/pgp.h -- UCTState::performTrICP (UCTState.cpp:137-139, 142-174, 194).  The
chain, every link a restatement the repository already pins:

  filter      oracle/preprocess_oracle.py unexplained_segment over the statics, EACH WITH ITS OWN MODEL (the reference
              reuses the newest object's model there, a slip the library does not copy); skipped without statics or
              with removal_radius <= 0; strict d2 < r * r with r * r a float32 product;
  compaction  the kept points in their original order;
  guess       G = rigid inverse of the pose: {R^T, -R^T t} in float64, -((a tx + b ty) + c tz), rounded once;
  ICP         tests/_icp_restate.py icp(kept, model, G, trim_fraction, energy_ratio, max_iterations): TrimmedICP form,
              k = (int)|trim * (float)n_kept| from the KEPT count;
  back        T = rigid inverse of the refined G by the same rule.

The library's own rules (PCL is not in the reference tree):
  k < 3 (n_kept == 0 included)   the state is left exactly as it came: T bit for bit, iters 0, energy 0;
  a bad state                    a non-finite pose, an unknown object or more than 16 statics: the host call refuses it,
                                 the device call gives a NaN T, iters -1, energy 0, n_kept 0 (`bad_state`);
  max_iterations <= 0            100; above 1000 refused;
  a model of 1 or 2 points       (`rotation_free`) every target coincides or lies on one line, so the rotation about it is
                                 not determined (Horn's matrix is rounding residue there): the refined pose is then any
                                 proper rigid transform that places the centroid of the selected source points on the
                                 centroid of their targets.  Distances to the model, and with them the pairs, n_kept, iters
                                 and the energy, do not depend on the choice and are held as everywhere.

`tricp_state` returns a dict: T (16,) float32, G (16,) float32 (the refined guess, camera -> object), energy float32,
iters, n_kept, keep (the filter's mask), k, touched.

MUTATIONS lists the wrong rules the scenes of tests/_tricp_scenes.py are built to tell from the right ones
(tests/test_tricp_restate_cpu.py shows that each does; tests/test_tricp_gpu.py holds the device to the unmutated chain)."""
import os
import sys

import numpy as np

import _icp_restate as I

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "oracle"))
import preprocess_oracle as po  # noqa: E402

f32, f64 = np.float32, np.float64
MAX_STATICS = 16

MUTATIONS = (
    "filter_le",         # the filter with d2 <= r * r
    "compact_reversed",  # the kept points compacted out of order (reversed)
    "k_unfiltered",      # k from the unfiltered segment's count
    "newest_model",      # each static with the newest object's model (the reference's slip)
    "skip",              # the refinement skipped: the pose goes back as it came
)

DEFAULTS = dict(trim_fraction=0.5, removal_radius=0.008, energy_ratio=1.0, max_iterations=100)


def rigid_inverse(m):
    """select.hip top_gather's rule on 16 column-major floats: float64, rounded once."""
    m = np.asarray(m, f32).reshape(16)
    t = m[12:15].astype(f64)
    o = np.zeros(16, f32)
    for r in range(3):
        a, b, c = (f64(m[4 * r]), f64(m[4 * r + 1]), f64(m[4 * r + 2]))
        o[r], o[4 + r], o[8 + r] = f32(a), f32(b), f32(c)
        with np.errstate(all="ignore"):
            o[12 + r] = f32(-((a * t[0] + b * t[1]) + c * t[2]))
    o[15] = 1
    return o


def _filter_le(seg, models, poses, radius):
    """unexplained_segment with <= for <: the mutation's own copy of the oracle's arithmetic"""
    seg = np.asarray(seg, f32)
    keep = np.ones(len(seg), bool)
    r2 = f32(radius) * f32(radius)
    for m, G in zip(models, np.asarray(poses, f32).reshape(-1, 16)):
        m = np.asarray(m, f32)
        p = [((G[r] * m[:, 0] + G[4 + r] * m[:, 1]) + G[8 + r] * m[:, 2]) + G[12 + r] for r in range(3)]
        dx, dy, dz = (seg[:, None, c] - p[c][None, :] for c in range(3))
        keep &= ~(((dx * dx + dy * dy) + dz * dz) <= r2).any(axis=1)
    return keep


def rotation_free(model):
    """the rule above: fewer than 3 model points leave the rotation undetermined"""
    return len(np.asarray(model).reshape(-1, 3)) < 3


def last_centroids(result, segment, model):
    """(centroid of the source points the last iteration selected, centroid of their targets), float64: what the refined
    guess maps onto what, whatever the rotation"""
    rec = result["trace"][-1]
    kept = np.asarray(segment, f32).reshape(-1, 3)[result["keep"]].astype(f64)
    tgt = np.asarray(model, f32).reshape(-1, 3).astype(f64)
    return kept[rec["pairs"]].mean(0), tgt[rec["j"][rec["pairs"]]].mean(0)


def bad_state():
    return dict(T=np.full(16, np.nan, f32), G=np.full(16, np.nan, f32), energy=f32(0), iters=-1, n_kept=0, keep=None, k=0,
                touched=True)


def tricp_state(segment, model, pose, statics=(), *, mutate=(), **opt):
    """One state: `segment` (n, 3) camera frame, `model` (m, 3) object frame, `pose` 16 floats column-major object ->
    camera, statics: a sequence of (static's model (q, 3), static's pose (16,)).  Options: DEFAULTS by name."""
    unknown = set(opt) - set(DEFAULTS)
    assert not unknown, unknown
    o = dict(DEFAULTS, **opt)
    mutate = (mutate,) if isinstance(mutate, str) else tuple(mutate)
    assert set(mutate) <= set(MUTATIONS), mutate
    seg = np.asarray(segment, f32).reshape(-1, 3)
    model = np.asarray(model, f32).reshape(-1, 3)
    pose = np.asarray(pose, f32).reshape(16).copy()
    statics = list(statics)
    max_it = int(o["max_iterations"])
    assert max_it <= 1000
    max_it = max_it if max_it > 0 else 100
    if not np.isfinite(pose).all() or len(statics) > MAX_STATICS:
        return bad_state()
    # ---- filter
    keep = np.ones(len(seg), bool)
    radius = f32(o["removal_radius"])
    if statics and radius > 0:
        models = [model if "newest_model" in mutate else np.asarray(m, f32).reshape(-1, 3) for m, _ in statics]
        poses = np.stack([np.asarray(T, f32).reshape(16) for _, T in statics])
        keep = (_filter_le if "filter_le" in mutate else po.unexplained_segment)(seg, models, poses, radius)
    # ---- compaction
    kept = seg[keep]
    if "compact_reversed" in mutate:
        kept = kept[::-1].copy()
    n_kept = len(kept)
    k = I.trim_count(o["trim_fraction"], len(seg) if "k_unfiltered" in mutate else n_kept) if n_kept else 0
    k = min(k, n_kept)
    out = dict(T=pose, G=rigid_inverse(pose), energy=f32(0), iters=0, n_kept=n_kept, keep=keep, k=k, touched=False)
    if k < 3 or "skip" in mutate:
        return out
    # ---- guess, ICP, back.  icp() derives k from trim_fraction and the count of the cloud it is given; the mutated k is
    # forced through a trim fraction that yields it
    tf = o["trim_fraction"]
    if "k_unfiltered" in mutate:
        tf = _trim_for(k, n_kept)
    G, e, it, trace = I.icp(kept, model, out["G"], trim_fraction=tf, energy_ratio=o["energy_ratio"], max_iterations=max_it)
    assert trace[0]["k"] == k, (trace[0]["k"], k)
    out.update(T=rigid_inverse(G), G=G, energy=e, iters=it, touched=True, trace=trace)
    return out


def _trim_for(k, n):
    """a float32 trim fraction in (0, 1] with trim_count(tf, n) == k"""
    if k >= n:
        return 1.0
    tf = f32((k + 0.5) / n)
    assert I.trim_count(tf, n) == k
    return float(tf)
