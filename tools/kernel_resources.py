#!/usr/bin/env python3
"""VGPRs / AGPRs / SGPRs / spills / occupancy / scratch of every kernel of the HIP library, each beside its budget
(tests/kernel_budgets.py), from the report the tests read (tests/kernel_report.py): the product's flags, device code only.
Arguments are passed to the compiler (the sweeps: `tools/kernel_resources.py -DRT_PT_WIDE_WAVES=5`).  No GPU needed."""
import os
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "tests")):
    sys.path.insert(0, p)
import kernel_budgets as B
import kernel_report as K

# column -> (report key, the limit kinds that bound it and how they print)
COLUMNS = (("VGPR", "VGPRs", {"vgprs_max": "<=", "vgprs_eq": "=="}), ("AGPR", "AGPRs", {}), ("SGPR", "TotalSGPRs", {"sgprs_max": "<="}),
           ("spill", "VGPRs Spill", {"vgpr_spill_max": "<="}), ("occ", "Occupancy [waves/SIMD]", {"waves_min": ">=", "waves_eq": "=="}),
           ("scratch", "ScratchSize [bytes/lane]", {"scratch_max": "<="}))

if K.hipcc_missing():
    sys.exit(K.hipcc_missing())
with tempfile.TemporaryDirectory() as tmp:
    report = K.library_report(tmp, sys.argv[1:])
    # the translation units beside rt_api.hip (the reflection sampler): their budget is tests/test_reflection_sample_budgets.py's
    import test_reflection_sample_budgets as S
    other = {}
    for unit in K.W._build.RT_SOURCES[1:]:
        other.update(K.compile_report(os.path.join(K.CSRC, unit), tmp, (K.W._build.INCLUDE,), sys.argv[1:]))
print("%-62s" % "kernel" + "".join(" %9s" % c[0] for c in COLUMNS) + "  note")
for name, res in report.items():
    rows = B.matching(name, B.ROWS)
    limits = B.ROWS[rows[0]] if rows else {}
    cells = ["%s%s" % (res.get(key), "".join(op + str(limits[k]) for k, op in kinds.items() if k in limits)) for _, key, kinds in COLUMNS]
    mark = ("; ".join(B.violations(limits, res)) if rows else "reference only" if B.matching(name, B.REFERENCES) else
            "unbudgeted" if B.matching(name, B.UNBUDGETED) else "NO ROW")
    print("%-62s" % name[:62] + "".join(" %9s" % c for c in cells) + "  " + mark)
for name, res in other.items():
    cells = ["%s" % res.get(key) for _, key, _ in COLUMNS]
    mark = "; ".join(B.violations(S.LIMITS, res)) if name in S.KERNELS else "NO ROW"
    print("%-62s" % name[:62] + "".join(" %9s" % c for c in cells) + "  reflection_sample.hip " + mark)
