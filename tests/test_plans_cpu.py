"""The plan queries answer what they answered when tests/golden/plans.json was recorded.

m324_gemm_plan / m324_attention_plan format the plan the launchers work from (csrc/gemm.hip make_plan, csrc/attention.hip
attn_plan); the model acts on the schedule number and every profile row is labelled with the text.  The fixture was recorded
from the library as it stood before launch and query were derived from one plan, so a changed answer is a changed launch.
Host-only: a child process with the devices hidden enumerates the cases (tests/golden/make_plan_table.py), which makes the
compute-unit count behind the persistent grids the library's fallback on every machine."""
import json
import os
import subprocess
import sys

from conftest import GOLDEN

sys.path.insert(0, GOLDEN)
import make_plan_table as table      # noqa: E402


def test_plan_queries_answer_as_recorded():
    with open(os.path.join(GOLDEN, "plans.json")) as f:
        want = json.load(f)
    # the switches come from m324_set_tunable alone: no M324_* of the caller's environment reaches the child (but the library's path)
    env = {k: v for k, v in os.environ.items() if not k.startswith("M324_") or k == "M324_LIB"}
    env.update(HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, os.path.join(GOLDEN, "make_plan_table.py"), "--stdout"], capture_output=True, text=True, env=env,
                       timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    got = json.loads(r.stdout)
    assert got["key"] == want["key"], "make_plan_table.py enumerates other cases than plans.json records: regenerate the fixture"
    bad = []
    for kind, cases in (("gemm", table.gemm_cases()), ("attn", table.attn_cases())):
        assert len(got[kind]) == len(want[kind])
        for i, case in enumerate(cases):
            g, w = got["plans"][got[kind][i]], want["plans"][want[kind][i]]
            if g != w:
                bad.append((kind, case, w, g))
    assert len(want["gemm"]) >= 7548 and len(want["attn"]) >= 2100 * 12
    assert not bad, f"{len(bad)} changed answers (case, recorded, now); the first: {bad[:5]}"
