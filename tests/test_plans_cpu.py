"""The plan queries answer what they answered when tests/golden/plans.json was recorded.

m324_gemm_plan / m324_attention_plan format the plan the launchers work from (csrc/gemm.hip make_plan, csrc/attention.hip
attn_plan); the model acts on the schedule number and every profile row is labelled with the text.  The fixture was recorded
from the library as it stood before the losing A/B switches of the attention launch path were retired (M324_LIB = the parent
commit's build), so a changed answer is a changed launch.
Host-only: a child process with the devices hidden enumerates the cases (tests/golden/make_plan_table.py), which makes the
compute-unit count behind the persistent grids the library's fallback on every machine."""
import os
import subprocess
import sys

from conftest import GOLDEN

sys.path.insert(0, GOLDEN)
import make_plan_table as table      # noqa: E402


def test_plan_queries_answer_as_recorded():
    with open(os.path.join(GOLDEN, "plans.json")) as f:
        want = table.loads(f.read())
    # the switches come from m324_set_tunable alone: no M324_* of the caller's environment reaches the child (but the library's path)
    env = {k: v for k, v in os.environ.items() if not k.startswith("M324_") or k == "M324_LIB"}
    env.update(HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, os.path.join(GOLDEN, "make_plan_table.py"), "--stdout"], capture_output=True, text=True, env=env,
                       timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    got = table.loads(r.stdout)
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


# what the launch switch of m324_attention builds (csrc/attention.hip M324_ATTN(...) and the frame-pair kernel)
ATTN_BUILT = {f"attn_bf16_kernel<{a}>" for a in (
    "false, 1, 4, false, 3", "false, 1, 8, false, 3", "false, 1, 4, true, 3", "false, 1, 8, true, 3",
    "true, 1, 4, false, 1", "true, 1, 4, false, 2", "true, 1, 4, false, 3", "true, 1, 4, true, 2", "true, 1, 4, true, 3",
    "true, 1, 8, false, 3", "true, 1, 8, true, 3")} | {"attn_frames_kernel<2, true>"}

_TUNABLES = """
import sys
sys.path.insert(0, sys.argv[1])
import make_plan_table as t
h = t.load_lib().load()
for name in sys.argv[2:]:
    assert h.m324_set_tunable(name.encode(), 1) == 0, name
    assert h.m324_set_tunable(name.encode(), -2 ** 31) == 0, name
for name in ("M324_ATTN_FLAT", "M324_ATTN_OCC", "M324_ATTN_NQ2"):
    assert h.m324_set_tunable(name.encode(), 1) < 0, name
"""


def test_retired_switches_are_refused_and_every_planned_attention_kernel_is_built():
    """m324_set_tunable knows exactly the library switches of switches.LIBRARY (the retired attention switches are unknown names),
    and the attention kernels the recorded plans name are the ones the launch switch instantiates: a plan that names another
    one is a call that fails with M324_ERR_UNSUPPORTED."""
    env = {k: v for k, v in os.environ.items() if not k.startswith("M324_") or k == "M324_LIB"}
    env.update(HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    from motion324_amd import switches
    r = subprocess.run([sys.executable, "-c", _TUNABLES, GOLDEN] + list(switches.LIBRARY), capture_output=True, text=True, env=env, timeout=60)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    with open(os.path.join(GOLDEN, "plans.json")) as f:
        want = table.loads(f.read())
    names = {want["plans"][i][1].split(" grid=")[0] for i in want["attn"]}
    assert {n for n in names if n.startswith(("attn_bf16_kernel<", "attn_frames_kernel<"))} == ATTN_BUILT
