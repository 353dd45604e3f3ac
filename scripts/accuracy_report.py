"""Walk tests/test_gpu_accuracy.py (the same walk: the tests themselves run) and write what they measured to
profiles/accuracy_routes.jsonl: e_rms and e_max of the kernel, of the baseline, their ratios (accuracy_util.measure) and the
device name.  One row per route, family or factorisation -- its measurement with the worst e_rms ratio, the number of
measurements ``n`` and the worst e_max ratio among them ``route_max_ratio``; ``--all`` writes one row per route, case,
quantity and input class instead (1260 rows, too many to keep in the repository).

    python scripts/accuracy_report.py [-o profiles/accuracy_routes.jsonl] [--all] [pytest arguments]

Exit status: pytest's.  Rows of failing checks are written too (a measurement is recorded before its bound is asserted)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-o", "--out", default=os.path.join(ROOT, "profiles", "accuracy_routes.jsonl"))
    ap.add_argument("--all", action="store_true", help="every measurement, not the worst of each route")
    args, rest = ap.parse_known_args()
    import pytest
    import torch
    os.chdir(ROOT)
    status = pytest.main(["tests/test_gpu_accuracy.py", "-q", "-s", "-p", "no:cacheprovider"] + rest)
    from tests import test_gpu_accuracy as ta
    device = "none"
    if torch.cuda.is_available():
        props = torch.cuda.get_device_properties(0)
        device = f"{props.name} ({getattr(props, 'gcnArchName', '?').split(':')[0]}, {props.multi_processor_count} CUs)"
    rows = ta.ROWS
    if not args.all:
        routes = {}
        for r in ta.ROWS:
            routes.setdefault(r["route"], []).append(r)
        rows = [dict(max(rs, key=lambda r: r["rms_ratio"]), n=len(rs), route_max_ratio=max(r["max_ratio"] for r in rs))
                for rs in routes.values()]
    with open(args.out, "w") as f:
        for r in rows:
            row = {k: (float(f"{v:.4g}") if isinstance(v, float) else v) for k, v in r.items()}
            f.write(json.dumps(dict(row, device=device)) + "\n")
    worst = {}
    for r in ta.ROWS:
        w = worst.setdefault(r["family"], [0.0, 0.0])
        w[0], w[1] = max(w[0], r["rms_ratio"]), max(w[1], r["max_ratio"])
    for fam, (a, b) in worst.items():
        print(f"{fam}: worst e_rms ratio {a:.2f}, worst e_max ratio {b:.2f}")
    print(f"{len(ta.ROWS)} measurements, {len(rows)} rows -> {args.out}")
    return int(status)


if __name__ == "__main__":
    sys.exit(main())
