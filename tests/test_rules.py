"""The decision functions of sgo_optimize_gn (sparse_gslam_amd/csrc/sgo_rules.h: when the multigrid hierarchy's coarse operators are
kept, refreshed, rebuilt, re-aggregated or reverted) are pure functions of iteration counts -- every rank of a multi-GPU run must
take the same decision from the same numbers.  tests/cpp/rules_unit.cpp checks them, and the per-call policy that drives them
(sgo_policy.h), on recorded count sequences; no GPU, no library."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_decision_functions_on_recorded_count_sequences(tmp_path):
    exe = tmp_path / "rules_unit"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "sparse_gslam_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "rules_unit.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    assert "rules ok" in out.stdout


def test_the_driver_uses_the_rules_header():
    """optimize_gn and its per-call policy hold no copy of a rule's arithmetic: the constants appear in sgo_rules.h only; the policy is
    host-only (sgo_rules.h and the standard library, no HIP header)."""
    csrc = os.path.join(ROOT, "sparse_gslam_amd", "csrc")
    src = open(os.path.join(csrc, "sgo_solve.cpp")).read()
    policy = open(os.path.join(csrc, "sgo_policy.h")).read()
    assert '#include "sgo_rules.h"' in src
    assert '#include "sgo_rules.h"' in policy
    for text in (src, policy):
        for literal in ("2 * call_best + 10", "4 * c->amg_best + 40", "85 * trial_old", "0.95 * c->amg_lag_slope",
                        "4 * c->hier.best + 40", "4 * g.best + 40", "0.95 * c->hier.lag_slope", "0.95 * g.lag_slope"):
            assert literal not in text, literal
        for pattern in (r"\b2 \* [\w.>-]*best \+ 10\b", r"\b4 \* [\w.>-]*best \+ 40\b", r"\b85 \* [\w.>-]*trial", r"\b0\.95 \* [\w.>-]*slope"):
            assert not re.search(pattern, text), pattern
    includes = re.findall(r'^\s*#\s*include\s*[<"]([^>"]+)[>"]', policy, re.M)
    assert includes and all(h == "sgo_rules.h" or "." not in h for h in includes), includes   # (standard headers have no extension)
    assert not any("hip" in h.lower() for h in includes), includes
