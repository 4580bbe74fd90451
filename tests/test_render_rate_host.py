"""tools/render_rate.py without a device: the cases of every family at its defaults (restated here from the loops of the
eleven tools it replaced), options, the JSON round trip of a case, --list's imports, and the stop at the first child that
fails."""

import importlib.util
import json
import os
import signal
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "render_rate.py")
_spec = importlib.util.spec_from_file_location("render_rate", TOOL)
render_rate = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(render_rate)

I = [1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0]
CJ = [-0.8, 0.156]
FOCUS = {"level": 8, "probe": 64, "dilate": 1}
FORMULAS = ["tricorn", "celtic", "buffalo", "perpendicular", "celtic-tricorn"]

# family -> (the fields that tell its cases apart, the cases in the order the family's old tool ran them)
EXPECTED = {
    "anti": (("what", "max_iter", "lockstep"),
             [(w, m, k) for m in (500, 20000) for w, k in (("anti product", False), ("anti lock-step", True))]),
    "focus": (("what", "max_iter", "lockstep", "focus", "batch", "max_batches"),
              [("normal", 20000, False, None, 128, 64), ("focus product", 20000, False, FOCUS, 4, 64),
               ("focus lock-step", 20000, True, FOCUS, 1, 4)]),
    "project": (("what", "max_iter", "lockstep", "projection", "batch", "max_batches"),
                [("normal", 20000, False, None, 128, 64), ("project product", 20000, False, I, 4, 64),
                 ("project lock-step", 20000, True, I, 1, 4)]),
    "power": (("what", "max_iter", "power", "lockstep"),
              [(w, m, d, k) for m in (500, 20000) for d in (3, 8)
               for w, k in (("power product", False), ("power lock-step", True))]),
    "julia": (("what", "max_iter", "julia", "projection", "lockstep"),
              [("julia product", 20000, [-1.0, 0.0], None, False), ("julia lock-step", 20000, [-1.0, 0.0], None, True),
               ("julia product", 20000, CJ, None, False), ("julia lock-step", 20000, CJ, None, True),
               ("projected product", 20000, None, I, False)]),
    "palette": (("what", "max_iter", "palette_planes", "projection", "julia"),
                [("projected, no palette", 2000, 0, I, None)]
                + [("projected palette, %d plane(s)" % n, 2000, n, I, None) for n in (1, 2, 3)]),
    "formula": (("what", "max_iter", "ship", "formula", "lockstep"),
                [("ship", 2000, True, None, False)] + [(f, 2000, False, f, False) for f in FORMULAS]
                + [("lockstep", 2000, False, "tricorn", True)]),
    "depth": (("what", "max_iter", "depth", "lockstep"),
              [row for m in (500, 20000) for row in [("projected product", m, None, False)]
               + [(w, m, ["cr", -2.0, 0.5, n], k) for n in (1, 64)
                  for w, k in (("depth product", False), ("depth lock-step", True))]]),
    "depth_palette": (("what", "max_iter", "depth", "depth_palette", "lockstep"),
                      [(w, m, ["cr", -2.0, 2.0, n], p, k) for m in (500, 20000) for n in (64, 256)
                       for w, p, k in (("depth product", False, False), ("depth-palette product", True, False),
                                       ("depth-palette lock-step", True, True))]),
    "frames": (("what", "max_iter", "julia", "sweep", "separate", "projection"),
               [(w % n if s else w, 2000, c, n, s, I) for c in (None, CJ) for n in (1, 8, 64)
                for w, s in (("frames render", False), ("%d separate renders", True))]),
    "phoenix": (("what", "max_iter", "julia", "phoenix", "lockstep", "max_batches"),
                [row for m in (500, 2000) for row in (
                    ("phoenix", m, None, [-0.5, 0.0], False, 64), ("phoenix_p0", m, None, [0.0, 0.0], False, 64),
                    ("julia", m, CJ, None, False, 64), ("phoenix_julia", m, CJ, [0.0, 0.0], False, 64),
                    ("lockstep", m, None, [-0.5, 0.0], True, 16))]),
}
COUNTS = {"anti": 4, "focus": 3, "project": 3, "power": 8, "julia": 5, "palette": 4, "formula": 7, "depth": 10,
          "depth_palette": 12, "frames": 12, "phoenix": 10}
# the setup fields and the families that may use each: everywhere else it says "the normal render"
SETUP = {"anti": {"anti"}, "ship": {"formula"}, "power": {"power"}, "formula": {"formula"}, "focus": {"focus"},
         "box": {"focus"}, "julia": {"julia", "frames", "phoenix"}, "phoenix": {"phoenix"},
         "depth": {"depth", "depth_palette"}, "depth_palette": {"depth_palette"}, "palette_planes": {"palette"},
         "sweep": {"frames"}, "separate": {"frames"}}


def listed(capsys, *argv):
    assert render_rate.main(list(argv) + ["--list"]) == 0
    return [json.loads(line) for line in capsys.readouterr().out.splitlines()]


@pytest.mark.parametrize("family", list(EXPECTED))
def test_default_cases_are_the_old_tools_cases_in_their_order(capsys, family):
    fields, want = EXPECTED[family]
    cases = listed(capsys, family)
    assert [tuple(c[f] for f in fields) for c in cases] == want
    assert len(cases) == COUNTS[family] and sum(COUNTS.values()) == 78 and set(COUNTS) == set(render_rate.FAMILIES)
    for c in cases:
        assert c["family"] == family and c["min_iter"] == 20 and c["side"] == (1024 if family == "frames" else 4096)
        assert c["seconds"] == 0.5 and c["reps"] == 3 and c["threads"] is None
        assert c["box"] == ([-0.2, 0.0, -0.9, -0.7] if family == "focus" else None)
        if c["what"] == "normal":
            assert (c["batch"], c["max_batches"]) == (128, 64)
        else:
            assert c["batch"] == (1 if c["lockstep"] else 4)
            assert c["max_batches"] == (64 if not c["lockstep"] else 16 if family == "phoenix" else 4)
        for f, families in SETUP.items():
            assert family in families or not c[f], (f, c)
        if family in ("anti", "focus") or c["what"] == "normal":
            assert c["projection"] is None and c["anti"] == (family == "anti")
        else:  # a plotted render: a fixed c on the identity plane, or a matrix
            assert (c["julia"] is not None and family != "frames") != (c["projection"] is not None), c


def test_options_reach_the_cases(capsys):
    cases = listed(capsys, "power", "--degrees", "5", "--max-iters", "100")
    assert [(c["power"], c["max_iter"], c["lockstep"]) for c in cases] == [(5, 100, False), (5, 100, True)]
    cases = listed(capsys, "project", "--skip-normal", "--skip-lockstep", "--project", "0,0,1,0:0,0,0,0x1p-1", "-m", "7",
                   "-c", "3", "--side", "64", "--threads", "1024", "--seconds", "0", "--reps", "1")
    assert len(cases) == 1 and cases[0]["projection"] == [0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.5]
    assert [cases[0][k] for k in ("max_iter", "min_iter", "side", "threads", "seconds", "reps")] == [7, 3, 64, 1024, 0.0, 1]
    cases = listed(capsys, "focus", "--box=-1,1,-1,1", "--level", "4", "--probe", "1", "--dilate", "0", "--lockstep-batch", "2")
    assert all(c["box"] == [-1.0, 1.0, -1.0, 1.0] for c in cases) and cases[2]["batch"] == 2
    assert cases[1]["focus"] == cases[2]["focus"] == {"level": 4, "probe": 1, "dilate": 0}
    cases = listed(capsys, "palette", "--planes", "2", "--julia=-1,0", "--max-iter", "50")
    assert [(c["what"], c["julia"], c["projection"], c["max_iter"]) for c in cases] == [
        ("julia palette, 2 plane(s)", [-1.0, 0.0], None, 50)]
    cases = listed(capsys, "depth_palette", "--kinds", "lockstep", "--slices", "4", "--window=-1:1", "--max-iters", "9")
    assert [(c["what"], c["depth"]) for c in cases] == [("depth-palette lock-step", ["cr", -1.0, 1.0, 4])]
    cases = listed(capsys, "frames", "--frames", "2", "--sources", "julia", "--plain-seconds", "0.25")
    assert [(c["sweep"], c["separate"], c["seconds"], c["julia"]) for c in cases] == [(2, False, 0.5, CJ), (2, True, 0.25, CJ)]
    assert [c["what"] for c in listed(capsys, "phoenix", "--renders", "lockstep,julia", "-m", "30")] == ["lockstep", "julia"]
    assert [c["what"] for c in listed(capsys, "formula", "--rows", "celtic")] == ["celtic"]
    assert [c["julia"] for c in listed(capsys, "julia", "--cs=0.25,0.5")] == [[0.25, 0.5]] * 2
    for bad in (["formula", "--rows", "nosuch"], ["depth_palette", "--kinds", "nosuch"], ["phoenix", "--renders", "nosuch"],
                ["project", "--project", "1,2,3"], ["nosuch"], []):
        with pytest.raises(SystemExit) as e:
            render_rate.main(bad + ["--list"] if bad else [])
        assert e.value.code == 2
        capsys.readouterr()


def test_default_limits():
    for family, (_, own) in render_rate.FAMILIES.items():
        limit = {**render_rate.COMMON, **own}["--limit"]
        assert limit == (240.0 if family in ("frames", "phoenix") else 120.0)


@pytest.mark.parametrize("family", list(EXPECTED))
def test_a_case_survives_the_trip_to_its_child(capsys, monkeypatch, family):
    """JSON -> the --one argument -> the case the child measures, unchanged; and the child is this tool, started fresh."""
    cases = listed(capsys, family, "--project", "0x1.8p-1,0,0,1e-300:0,0.1,0,0") if family == "project" else listed(capsys, family)
    started, measured = [], []
    monkeypatch.setattr(render_rate, "run_children", lambda commands, limit: started.extend(commands) or 0)
    monkeypatch.setattr(render_rate, "measure", lambda case: measured.append(case) or {})
    args = [family] + (["--project", "0x1.8p-1,0,0,1e-300:0,0.1,0,0"] if family == "project" else [])
    assert render_rate.main(args) == 0
    assert len(started) == len(cases)
    for (label, argv), case in zip(started, cases):
        assert argv[:3] == [sys.executable, TOOL, "--one"] and len(argv) == 4 and case["what"] in label
        assert render_rate.main(argv[2:]) == 0
    assert measured == cases


def test_list_stays_off_the_device():
    code = ("import sys; sys.path.insert(0, %r); import render_rate\n"
            "for f in render_rate.FAMILIES:\n"
            "    assert render_rate.main([f, '--list']) == 0\n"
            "assert 'torch' not in sys.modules and 'cudabrot_amd' not in sys.modules\n" % os.path.dirname(TOOL))
    r = subprocess.run([sys.executable, "-c", code], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]
    assert len(r.stdout.splitlines()) == 78


def child(code):
    return [sys.executable, "-c", code]


def test_run_children_stops_at_the_first_failure(tmp_path, capfd):
    marker = tmp_path / "started"
    touch = ("touch", child("open(%r, 'w').close()" % str(marker)))
    assert render_rate.run_children([("fine", child("pass")), ("three", child("import sys; sys.exit(3)")), touch], 30) == 3
    assert not marker.exists() and "three ended with status 3" in capfd.readouterr().out
    assert render_rate.run_children([("slow", child("import time; time.sleep(30)")), touch], 1) == 124
    assert not marker.exists() and "slow ran past 1 s" in capfd.readouterr().out
    killed = child("import os, signal; os.kill(os.getpid(), signal.SIGKILL)")
    assert render_rate.run_children([("killed", killed), touch], 30) == 128 + signal.SIGKILL
    assert not marker.exists() and "killed ended with status -9" in capfd.readouterr().out
    assert render_rate.run_children([("fine", child("pass")), touch], 30) == 0 and marker.exists()
