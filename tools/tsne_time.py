"""Time, peak memory and accuracy of the exact t-SNE behind demo_tsne (utils/tsne.py): the kernels of libdcl_tsne.so against the
torch composition of the same commit, on the same GPU and in the same process, HIP-event medians.

    python tools/tsne_time.py [--runs 10] [--iters 100] [--sizes 19000,4000] [--out profiles/tsne_time.json]
                              [--accuracy-out profiles/tsne_accuracy.json]

Per size (D = 50, perplexity 30, clustered random features): ``iters`` iterations from the start state (early exaggeration, KL
every tenth iteration), ``dts_cond_p`` on its own against the composition's ``cond_p`` (the composition ``--cond-runs`` times: it
takes seconds), and ``dts_gradient`` on its own with its share of 8 TB/s (N * N * 4 bytes per launch).  Peak memory is what a
call allocates beyond P and its inputs.  The accuracy pass repeats the measurements of tests/test_tsne_hip.py on their inputs and
writes the observed figures next to the float32 composition's.  Every part runs in a child process of its own under its own
time limit; the first one that fails or runs out of time ends the run.  Not a test: nothing is asserted about the ratios."""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_BYTES_PER_S = 8e12


def timed(fn, warmup, runs, dev, reset=None):
    import torch
    for _ in range(warmup):
        if reset:
            reset()
        fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    ms = []
    for _ in range(runs):
        if reset:
            reset()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "runs": runs,
            "peak_mib": (torch.cuda.max_memory_allocated(dev) - base) / 2 ** 20}


def features(n, d, dev):
    import torch
    g = torch.Generator().manual_seed(n)
    centres = 4 * torch.randn(19, d, generator=g)
    return (centres[torch.arange(n) % 19] + torch.randn(n, d, generator=g)).to(dev)


def child_size(a):
    import torch
    import mscs_amd  # noqa: F401
    from mscs_amd import _lib_tsne as lt
    from mscs_amd.utils import tsne as T
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda:0")
    n, d, u = a.child_size, 50, 30.0
    assert lt.supported(n, d, u)
    X, plan = features(n, d, dev), lt.plan(n)
    res = {"N": n, "D": d, "perplexity": u, "iters": a.iters}
    P, beta = torch.empty(n, n, device=dev), torch.empty(n, device=dev)
    res["cond_p_hip"] = timed(lambda: lt.cond_p(X, u, P, beta), 1, a.runs, dev)
    res["cond_p_torch"] = timed(lambda: T.cond_p(X, u), 0, a.cond_runs, dev)
    res["cond_p_torch"]["peak_mib"] -= n * n * 4 / 2 ** 20                             # (its P is an output, as P above)
    part = torch.empty(plan["sym_groups"], device=dev)
    Pc = torch.empty_like(P)
    res["symmetrize_hip"] = timed(lambda: lt.symmetrize(Pc, part), 1, a.runs, dev, reset=lambda: Pc.copy_(P))
    lt.symmetrize(P, part)
    del Pc
    Y0 = T.initial_embedding(n, 0).to(dev)
    Y, iY, gains, dY = (torch.empty_like(Y0) for _ in range(4))
    ws, kl = torch.empty(plan["ws_floats"], device=dev), torch.zeros(a.iters // 10, device=dev)

    def reset():
        Y.copy_(Y0), iY.zero_(), gains.fill_(1.0)
    res["iterations_hip"] = timed(lambda: lt.run(P, Y, iY, gains, dY, ws, 0, a.iters, kl), 1, a.runs, dev, reset)
    y_hip, kl_hip = Y.clone(), kl.clone()
    res["iterations_torch"] = timed(lambda: T.iterate_(P, Y, iY, gains, 0, a.iters, kl), 1, a.runs, dev, reset)
    res["kl_last"] = {"hip": float(kl_hip[-1]), "torch": float(kl[-1])}
    res["y_rel_diff_after_iters"] = float((y_hip - Y).abs().max() / Y.abs().max())
    zpart = ws[:plan["z_parts"]]
    lt.zsum(Y, zpart)
    g = timed(lambda: lt.gradient(P, Y, 1.0, zpart, dY), 2, 20, dev)
    g["bytes_per_s"] = n * n * 4 / (g["median_ms"] * 1e-3)
    g["fraction_of_8TBps"] = g["bytes_per_s"] / HBM_BYTES_PER_S
    res["gradient_hip"] = g
    res["zsum_hip"] = timed(lambda: lt.zsum(Y, zpart), 2, 20, dev)
    res["speedup_iterations"] = res["iterations_torch"]["median_ms"] / res["iterations_hip"]["median_ms"]
    res["speedup_cond_p"] = res["cond_p_torch"]["median_ms"] / res["cond_p_hip"]["median_ms"]
    print("RESULT " + json.dumps(res))


def child_accuracy(a):
    """the figures of tests/test_tsne_hip.py, observed (err) next to the float32 composition's (e32)"""
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import mscs_amd  # noqa: F401
    import _tsne_cases as cases
    from mscs_amd import _lib_tsne as lt
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda:0")
    new = lambda *shape: torch.empty(shape, device=dev)                                # noqa: E731
    rows = []
    for case in cases.CASES:
        n, d, s = case
        X, u, ref = cases.make_x(n, d, s), cases.perplexity_for(n), cases.cond_reference(n, d, s)
        P, beta = new(n, n), new(n)
        lt.cond_p(X.to(dev), u, P, beta)
        P64, H = cases.p_at_beta(X, beta.cpu())
        row = {"case": cases.case_id(case), "cond_p": {"err": cases.rel_max(P, P64, dim=1), "e32": ref["e32"],
                                                       "residual": float((H - math.log(u)).abs().max()), "residual_f32": ref["res32"],
                                                       "beta_min": float(beta.min()), "beta_max": float(beta.max())}}
        sref = cases.sym_reference(*case)
        S = sref["P"].to(dev).clone()
        lt.symmetrize(S, new(lt.plan(n)["sym_groups"]))
        row["symmetrize"] = {"err": cases.rel_max(S, sref["S64"]), "e32": sref["e32"]}
        Pg, Yg = (t.to(dev) for t in cases.grad_state(*case))
        plan = lt.plan(n)
        for ex in (4.0, 1.0):
            gref = cases.grad_reference(*case, ex)
            zpart, klpart, dY, z_out, kl_out = new(plan["z_parts"]), new(plan["grad_groups"]), new(n, 2), new(1), new(1)
            lt.zsum(Yg, zpart)
            lt.gradient(Pg, Yg, ex, zpart, dY, klpart, z_out)
            lt.update(dY.clone(), *[torch.zeros(n, 2, device=dev) for _ in range(3)], 0.5, new(2 * plan["upd_groups"]), klpart, kl_out)
            row[f"gradient_ex{int(ex)}"] = {"dY": cases.rel_max(dY, gref["dY"]), "dY_e32": gref["e_dY"],
                                            "Z": abs(float(z_out) - gref["Z"]) / gref["Z"], "Z_e32": gref["e_Z"],
                                            "KL": abs(float(kl_out) - gref["KL"]) / abs(gref["KL"]), "KL_e32": gref["e_KL"],
                                            "floor": cases.floor(n)}
        rows.append(row)
    upd = []
    for n in cases.NS:
        for mom in (0.5, 0.8):
            ref = cases.update_reference(n, mom)
            dY, iY, gains, Y = (t.to(dev).clone() for t in cases.update_inputs(n))
            lt.update(dY, iY, gains, Y, mom, new(2 * lt.plan(n)["upd_groups"]))
            upd.append({"N": n, "momentum": mom, "gains_equal": bool(torch.equal(gains.cpu(), ref[cases.F32][1])),
                        "iY": cases.rel_max(iY, ref[cases.F64][0]), "iY_e32": ref["e_iY"], "Y": cases.rel_max(Y, ref[cases.F64][2]),
                        "Y_e32": ref["e_Y"], "floor": cases.floor(n)})
    from mscs_amd.utils import tsne_exact
    Xc, labels = cases.clusters()
    Yc, kl = tsne_exact(Xc.to(dev), 30, 250, 0)
    outcome = {"kl_110": float(kl[10]), "kl_250": float(kl[24]), "purity": cases.purity(Yc, labels)}
    print("RESULT " + json.dumps({"cases": rows, "update": upd, "outcome": outcome}))


def run_child(args, limit):
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, capture_output=True, text=True, timeout=limit)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit(f"child {args} failed with {r.returncode}")
    line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--cond-runs", type=int, default=3)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--sizes", default="19000,4000")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tsne_time.json"))
    ap.add_argument("--accuracy-out", default=os.path.join(ROOT, "profiles", "tsne_accuracy.json"))
    ap.add_argument("--limit", type=int, default=420, help="seconds per child")
    ap.add_argument("--child-size", type=int, default=0)
    ap.add_argument("--child-accuracy", action="store_true")
    a = ap.parse_args()
    if a.child_size:
        return child_size(a)
    if a.child_accuracy:
        return child_accuracy(a)
    common = ["--runs", str(a.runs), "--cond-runs", str(a.cond_runs), "--iters", str(a.iters)]
    if a.accuracy_out:
        acc = run_child(["--child-accuracy"], a.limit)
        os.makedirs(os.path.dirname(a.accuracy_out), exist_ok=True)
        with open(a.accuracy_out, "w") as f:
            json.dump(acc, f, indent=1)
            f.write("\n")
        print(f"wrote {a.accuracy_out}: outcome {acc['outcome']}")
    out = {"what": "exact t-SNE: libdcl_tsne.so against the torch composition (tools/tsne_time.py)", "sizes": []}
    for n in [int(v) for v in a.sizes.split(",") if v]:
        res = run_child(common + ["--child-size", str(n)], a.limit)
        out["sizes"].append(res)
        print(f"N = {n}: {a.iters} iterations {res['iterations_hip']['median_ms']:.1f} ms (torch {res['iterations_torch']['median_ms']:.1f} ms), "
              f"cond_p {res['cond_p_hip']['median_ms']:.1f} ms (torch {res['cond_p_torch']['median_ms']:.1f} ms), "
              f"gradient {res['gradient_hip']['median_ms']:.3f} ms = {res['gradient_hip']['fraction_of_8TBps']:.2f} of 8 TB/s", flush=True)
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
