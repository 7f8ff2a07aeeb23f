"""The plan of the wave-per-packet calls (yu::plan_wave, yustack_amd/csrc/yucsum_plan.h):
tests/golden/wave_plans.txt holds what yu::plan_iov, yu::plan_iov_pack and yu::plan_build
returned before the one table replaced them (recorded from their printers; k_build4, then
row 0 of its own enum, written as row 8), one line `family n mode fill cus | env | kernel
policy blocks name` per case: iov and pack for mode 0..9 x fill 0, 1 x n 1, 5, 4097, 2^20
x 64, 256, 304 CUs, build for the same n x CUs, each with no knobs, with knobs behind the
closed gate and under three YU_TUNING=1 sets. The split lines at its end are what
yu::plan_split returned for the same n x CUs x knobs before k_split became row 9 of the
table (recorded from its printer, which had no kernel id: written as row 9).
tests/cpp/wave_plan.cpp reproduces every line. CPU only."""
import os

import wave_plan
from test_plan import ROOT

GOLDEN = os.path.join(ROOT, "tests", "golden", "wave_plans.txt")


def test_wave_plans_match_the_record():
    want = open(GOLDEN).read().splitlines()
    by_env = {}
    for k, line in enumerate(want):
        case, env, _ = line.split(" | ")
        by_env.setdefault(env, []).append((k, case.split()))
    assert len(want) == 5 * (2 * 10 * 2 * 4 * 3 + 4 * 3 + 4 * 3) and len(by_env) == 5
    for env, cases in by_env.items():
        e = dict(kv.split("=") for kv in env.split()) if env != "-" else None
        got = wave_plan.run([x for _, c in cases for x in c], e)
        assert len(got) == len(cases)
        for (k, c), g in zip(cases, got):
            assert f"{' '.join(c)} | {env} | {g}" == want[k], f"wave_plans.txt:{k + 1}: the plan changed"
    # every row of the table is planned somewhere in the record
    assert {line.split(" | ")[2].split()[0] for line in want} == {str(k) for k in range(10)}
    assert wave_plan.enum() == list(range(11))
