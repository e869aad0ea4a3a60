"""Device time of PPF Hough voting (pgp_ppf_vote_device) and of pgp_ppf_hypotheses (vote + LCP scoring, one call).

    python tools/ppf_time.py [calls] [out]

Two segments against the drop-in's 800-point search model: the drop-in's own (tests/_dropin.make_dropin_case sizes: the
visible object plus 1500 clutter points, 2043 points, 18 682 keys) and a 10 000-point segment.  Default options
(ref_step 5, 30 bins, one peak per reference point); the LDS accumulator path and the HBM path (PGP_PPF_ACC=hbm).
pgp_ppf_vote_device is timed with HIP events around each call after a warm-up, median of `calls` (>= 20);
pgp_ppf_hypotheses with the host clock (it is synchronous).  The report goes to stdout and to `out`
(default profiles/ppf_time.txt)."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

from _dropin import ppf_map  # noqa: E402
from _ppf_restate import table_arrays  # noqa: E402
from physimglobalpose_amd import LcpScorer, synth  # noqa: E402
from physimglobalpose_amd._lib import PGP_MODE_WEIGHTED  # noqa: E402


def segment(n_scene, clutter, config_id):
    w = synth.make_workload(n_scene, 1500, 4, config_id=config_id, n_search=800)
    rng = np.random.default_rng(0)
    obj = np.flatnonzero(w.P_w == 1.0)
    cl = rng.choice(np.flatnonzero(w.P_w < 1.0), min(clutter, int((w.P_w < 1.0).sum())), replace=False)
    keep = np.sort(np.concatenate([obj, cl]))
    return w, keep


def main():
    calls = max(20, int(sys.argv[1]) if len(sys.argv) > 1 else 50)
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "ppf_time.txt")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    cases = {"drop-in segment": segment(8000, 1500, 91)}
    w10, keep10 = segment(50000, 9500, 91)
    cases["10k-point segment"] = (w10, keep10[np.linspace(0, len(keep10) - 1, 10000).astype(int)])
    st = torch.cuda.Stream()
    say(f"PPF voting, default options (ref_step 5, 30 bins, 1 peak), median of {calls} calls")
    for name, (w, keep) in cases.items():
        sc = LcpScorer(0)
        P, N, W = w.P_xyz[keep], w.P_nrm[keep], w.P_w[keep]
        table = ppf_map(w.Qs_xyz, w.Qs_nrm)
        keys, counts, pairs = table_arrays(table)
        sc.set_scene(P, N, W, w.delta)
        sc.set_model(w.Q_xyz, w.Q_nrm)
        sc.set_ppf_map(keys, counts, pairs)
        sc.set_ppf_model(w.Qs_xyz, w.Qs_nrm)
        n_hyp = sc.ppf_vote()[4]
        for acc in ("lds", "hbm"):
            if acc == "hbm":
                os.environ["PGP_PPF_ACC"] = "hbm"
            with torch.cuda.stream(st):
                bufs = sc.ppf_vote_device(stream=st)
                for _ in range(5):
                    sc.ppf_vote_device(d_T=bufs[0], d_votes=bufs[1], d_ref=bufs[2], d_cell=bufs[3],
                                       d_n_out=bufs[4], stream=st)
                ts = []
                for _ in range(calls):
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record(st)
                    sc.ppf_vote_device(d_T=bufs[0], d_votes=bufs[1], d_ref=bufs[2], d_cell=bufs[3], d_n_out=bufs[4],
                                       stream=st)
                    b.record(st)
                    b.synchronize()
                    ts.append(a.elapsed_time(b))
            hs = []
            for mode in (0, PGP_MODE_WEIGHTED):
                sc.ppf_hypotheses(mode)
                t = []
                for _ in range(calls):
                    t0 = time.perf_counter()
                    sc.ppf_hypotheses(mode)
                    t.append(time.perf_counter() - t0)
                hs.append(np.median(t) * 1e3)
            os.environ.pop("PGP_PPF_ACC", None)
            say(f"  {name:18s} scene {len(P):6d} pts, model {len(w.Qs_xyz)} pts, {len(keys)} keys, {len(pairs)} pairs, "
                f"{n_hyp} hypotheses, accumulator {acc}: pgp_ppf_vote_device {np.median(ts) * 1e3:8.1f} us "
                f"(min {np.min(ts) * 1e3:7.1f});  pgp_ppf_hypotheses (host wall clock) plain {hs[0]:.3f} ms, "
                f"weighted {hs[1]:.3f} ms")
        sc.close()
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
