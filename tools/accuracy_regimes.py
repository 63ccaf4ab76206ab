"""The device's measured accuracy over the hyper-parameter regimes of tests/golden/regimes.json, as a record (not a threshold).

  python tools/accuracy_regimes.py [--out profiles/accuracy_regimes.jsonl]

Runs the comparisons of tests/test_gpu_regimes.py (handles against the 50-digit truths, and the appends of the corner subset) and
writes, per model, size and output, the worst err/(B·scale) over the grid — B = cond(K)·rows·2⁻⁵³, the unit in which the bars are
8 (logpdf, μ, var) and 100 (gradients) — with the case that attains it, beside the fp64 oracle's own worst ratio from the fixture's
header.  One line per (model, size); a last line per model holds the oracle's figures.  Lines marked "fixture": "regimes_more" hold
the same for the further truths of tests/golden/regimes_more.json (tests/test_gpu_regimes_more.py), with the multipliers of their bars."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "accuracy_regimes.jsonl"))
    args = ap.parse_args()
    import __graft_entry__ as entry
    entry.build()
    from boss_jl_amd import api
    import regimes_cases as R
    api.load_library()
    fx = R.load()
    lines = []
    for model in ("plain", "grad", "gibbs"):
        for data in fx[model]["datasets"]:
            worst, worst_app = {}, {}

            def note(tab, r, name):
                for k, v in r.items():
                    if v >= tab.get(k, (-1.0, ""))[0]:
                        tab[k] = (v, name)

            cs = [c for c in fx[model]["cases"] if c["data"] == data]
            for c in cs:
                for what, got, keep in R.DEVICE[model](api, fx, c):
                    note(worst, R.ratios(c, got, model, keep), c["name"])
                if R.is_corner(model, c):
                    for one_by_one in (False, True):
                        got, keep = R.device_append(api, model, fx, c, one_by_one)
                        note(worst_app, R.ratios(c, got, model, keep), c["name"])
            D = fx[model]["datasets"][data]
            line = {"model": model, "size": data, "d": int(D["X"].shape[0]), "points": int(D["X"].shape[1]), "rows": cs[0]["rows"], "cases": len(cs),
                    "cond_max": max(c["cond"] for c in cs), "bars": {"logpdf": 8, "mu": 8, "var": 8, "gradients": 100},
                    "worst_err_over_B": {k: {"ratio": float(f"{v:.3e}"), "case": n} for k, (v, n) in worst.items()},
                    "worst_err_over_B_append": {k: {"ratio": float(f"{v:.3e}"), "case": n} for k, (v, n) in worst_app.items()}}
            print(json.dumps(line), flush=True)
            lines.append(line)
        lines.append({"model": model, "oracle_worst_err_over_B": fx["header"]["oracle_worst_ratio"][model]})
    # the further truths of tests/golden/regimes_more.json (tests/test_gpu_regimes_more.py): covariances, the gradient-observation and
    # Gibbs candidate gradients, program-kernel posteriors.  Their multipliers were chosen from the oracle alone, so the device's margin
    # shows here: the worst ratio per quantity beside the multiplier of its bar.
    import boss_jl_amd as B
    fxm = R.load_more()
    progs = R.kprog_programs(B)
    for model in R.MODELS_MORE:
        limit = R.limit_more(fxm, model)
        for data in fx["plain" if model == "kprog" else model]["datasets"]:
            worst = {}
            cs = [c for c in fxm[model] if c["data"] == data]
            for c in cs:
                for what, got, keep in R.DEVICE_MORE[model](api, fx, c, progs=progs):
                    for k, v in R.ratios(c, got, model, keep).items():
                        if v >= worst.get(k, (-1.0, ""))[0]:
                            worst[k] = (v, c["name"])
            D = fx["plain" if model == "kprog" else model]["datasets"][data]
            line = {"fixture": "regimes_more", "model": model, "size": data, "d": int(D["X"].shape[0]), "points": int(D["X"].shape[1]),
                    "rows": cs[0]["rows"], "cases": len(cs), "cond_max": max(c["cond"] for c in cs), "bars": {k: limit[k] for k in worst},
                    "worst_err_over_B": {k: {"ratio": float(f"{v:.3e}"), "case": n} for k, (v, n) in worst.items()}}
            print(json.dumps(line), flush=True)
            lines.append(line)
        lines.append({"fixture": "regimes_more", "model": model, "oracle_worst_err_over_B": fxm["header"]["oracle_worst_ratio"][model],
                      "multiplier": fxm["header"]["multiplier"][model]})
    with open(args.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
