"""tools/step_digest.py in deterministic mode prints the same line in two fresh processes (three BAT steps, the last one a
replayed HIP graph)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CMD = [sys.executable, os.path.join(ROOT, "tools", "step_digest.py"), "--model", "BAT", "--batch", "2", "--template", "256",
       "--search", "512", "--steps", "3", "--graph", "--deterministic"]


def _run():
    p = subprocess.run(CMD, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=240)
    assert p.returncode == 0, (p.returncode, p.stderr[-2000:])
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return lines[0]


def test_two_processes_print_the_same_digests():
    first = _run()                      # (its exit status is checked before the second process starts)
    second = _run()
    d = json.loads(first)
    assert d["deterministic"] is True and d["graph"] is True and len(d["losses"]) == 3
    assert len(d["grads"]) > 20 and sum(v != "none" for v in d["grads"].values()) > 20 and len(d["state"]) > len(d["grads"])
    assert len(set(d["losses"])) == 3   # three batches, three losses
    assert first == second
