"""Walk tests/test_gpu_thresholds.py once (the same walk: the tests themselves run) and write what every side that ran
measured to profiles/thresholds.jsonl: the entry, its site and guard, the case, the route words of its plan, the bytes it
planned and the peak torch.cuda.max_memory_allocated() saw, its seconds (inputs, launch, truth and the full check) and its
worst error as a fraction of the bound (route_util.TOL32 x max|want|), with the device name.

    python scripts/threshold_report.py [-o profiles/thresholds.jsonl] [pytest arguments]

Exit status: pytest's.  Rows of failing checks are not written (a side is recorded once its check has passed)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-o", "--out", default=os.path.join(ROOT, "profiles", "thresholds.jsonl"))
    args, rest = ap.parse_known_args()
    import pytest
    import torch
    os.chdir(ROOT)
    status = pytest.main(["tests/test_gpu_thresholds.py", "-q", "-p", "no:cacheprovider"] + rest)
    from tests import test_gpu_thresholds as tt
    device = "none"
    if torch.cuda.is_available():
        props = torch.cuda.get_device_properties(0)
        device = f"{props.name} ({getattr(props, 'gcnArchName', '?').split(':')[0]}, {props.multi_processor_count} CUs)"
    with open(args.out, "w") as f:
        for r in tt.ROWS:
            row = {k: (float(f"{v:.4g}") if isinstance(v, float) else v) for k, v in r.items()}
            f.write(json.dumps(dict(row, device=device)) + "\n")
        for (entry, side), how in tt.DONE.items():
            if how != "ran":
                f.write(json.dumps(dict(entry=entry, side=side, outcome=how, device=device)) + "\n")
    print(f"{len(tt.ROWS)} sides ran, {len(tt.DONE) - len(tt.ROWS)} refused, plan-only or skipped -> {args.out}")
    return int(status)


if __name__ == "__main__":
    sys.exit(main())
