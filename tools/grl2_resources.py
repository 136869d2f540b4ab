#!/usr/bin/env python3
"""Registers, scratch and occupancy of the step kernel ``beat.models.from_ode`` generates for the test models, GRL1 beside GRL2:
each model's plain and pending-update instances cross-compiled for gfx950 (no GPU needed) with the flags the library compiles
a registered model with, read by tools/kernel_resources.py.

    python3 tools/grl2_resources.py [--md profiles/table.md]
"""
import argparse
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "fenicsx-beat_amd"))
sys.path.insert(0, str(ROOT / "tools"))

from kernel_resources import resource_rows  # noqa: E402

SCHEMES = ("generalized_rush_larsen", "generalized_rush_larsen_2")


def main():
    from beat.models import from_ode

    ap = argparse.ArgumentParser()
    ap.add_argument("--md", default=None)
    ap.add_argument("files", nargs="*", default=[str(ROOT / "tests" / "data" / f"{stem}.ode") for stem in ("small_cell", "language_cell", "big_cell")])
    args = ap.parse_args()
    lines = ["| model | scheme | instance | VGPRs | AGPRs | scratch B/lane | waves/SIMD | SGPRs | spilled SGPRs |", "|---|---|---|---:|---:|---:|---:|---:|---:|"]
    with tempfile.TemporaryDirectory() as tmp:
        for path in args.files:
            for scheme in SCHEMES:
                model = from_ode(path, scheme=scheme)
                for tag, inst in (("plain", "false, false"), ("pending update", "false, true")):
                    unit = Path(tmp) / f"{model.cxx_name}_{tag.split()[0]}.hip"
                    unit.write_text('#include "beat_ode_kernel.h"\n' + model.source +
                                    f"\ntemplate __global__ void ode_step_kernel<{model.cxx_name}, {inst}>(\n    double*, int64_t, int64_t, "
                                    f"ParamPack<{model.cxx_name}::NP>, typename {model.cxx_name}::Derived, const double*, int64_t, double, double, int, "
                                    "double*, PendingV, MarkedArgs, SparseRows);\n")
                    for r in resource_rows(unit, extra=["-mllvm", "-disable-machine-licm", "-w"], name_filter="ode_step_kernel"):
                        lines.append(f"| {Path(path).stem} | {scheme} | {tag} | " + " | ".join(str(v) for v in r[1:7]) + " |")
                        print(lines[-1], flush=True)
    text = "\n".join(lines)
    if args.md:
        Path(args.md).write_text(text + "\n")


if __name__ == "__main__":
    main()
