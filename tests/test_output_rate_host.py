"""tools/output_rate.py without a device: the rows are those of the three tools it replaced, every one in both trees;
the children alternate, each size twice per tree; the record's header is formed; --list imports neither the library nor
torch; and the first child that fails, or runs past its limit, ends the run with nothing started after it."""

import importlib.util
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "output_rate.py")
_spec = importlib.util.spec_from_file_location("output_rate", TOOL)
output_rate = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(output_rate)

# the rows, restated: the image call as each flag sets it, the device calls under them, the copy as the yardstick
ROWS = {
    "grayscale_image unflagged", "grayscale_image --white-clip 0.1", "grayscale_image equalised",
    "grayscale_image --density-filter 4", "grayscale_image --density-filter 8", "grayscale_image unflagged again",
    "white_count_device p=0 (one sweep)", "white_count_device p=0.1", "equalize_bins_device (one sweep)",
    "tone_map_device, table form (whole call)", "tone_map_device_equalized (whole call)",
    "density_filter_device R=4 (with its maximum pass)", "density_filter_device R=8 (with its maximum pass)",
    "device copy of 8n bytes (read + write)",
}


def test_the_case_list_is_complete():
    assert len(output_rate.ROWS) == len(ROWS) == 14 and set(output_rate.ROWS) == ROWS
    assert output_rate.ROWS[0] == "grayscale_image unflagged" and output_rate.ROWS[-1] == "grayscale_image unflagged again"
    assert output_rate.children("/p", [4096, 16384]) == [
        (which, root, size) for size in (4096, 16384)
        for which, root in (("current", ROOT), ("parent", "/p"), ("current", ROOT), ("parent", "/p"))]
    assert [output_rate.passes(s) for s in (1024, 4096, 4097, 16384)] == [64, 64, 32, 32]
    assert output_rate.child_command("/p", "parent", 4096) == [sys.executable, TOOL, "child", "/p", "parent", "4096"]
    assert (output_rate.REPS, output_rate.GAMMA, output_rate.CLIP, output_rate.RADII) == (3, 2.2, 0.1, (4, 8))


def test_the_record_s_header_is_formed():
    head = output_rate.header("one MI355X, 2026-10-21", [4096, 16384])
    lines = head.splitlines()
    assert lines[0] == ("# tools/output_rate.py on one MI355X, 2026-10-21, sizes 4096 and 16384, window W = 8192 "
                        "(DESIGN.md 4.24-4.26):")
    assert len(lines) == 4 and all(line.startswith("# ") for line in lines) and head.endswith("\n")
    assert "`current`" in head and "`parent`" in head and "every row in both" in head


def test_list_stays_off_the_library_and_the_device():
    code = ("import sys; sys.path.insert(0, %r); import output_rate\n"
            "assert output_rate.main(['--list', '4096', '16384']) == 0\n"
            "assert 'torch' not in sys.modules and 'cudabrot_amd' not in sys.modules and 'numpy' not in sys.modules\n"
            % os.path.dirname(TOOL))
    r = subprocess.run([sys.executable, "-c", code], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]
    out = r.stdout.splitlines()
    assert out[:4] == output_rate.header("WHERE", [4096, 16384]).splitlines()
    listed = [json.loads(line) for line in out[4:]]
    assert [c["what"] for c in listed[:14]] == output_rate.ROWS
    assert [(c["child"], c["size"], c["passes"]) for c in listed[14:]] == [
        (which, size, passes) for size, passes in ((4096, 64), (16384, 32)) for which in ("current", "parent") * 2]


def line(which, size, what, reps):
    return json.dumps({"what": what, "which": which, "size": size, "reps_s": reps})


def stub(tmp_path, fail_at=None, status=3):
    """A child command that needs no GPU: it notes that it was started, prints one row, and fails where it is told to."""
    def command(root, which, size):
        code = ("import sys; open(%r, 'a').write(%r); print(%r, flush=True); sys.exit(%d)"
                % (str(tmp_path / "started"), "%s %d\n" % (which, size),
                   line(which, size, "a row", [1.0, 2.0, 3.0] if which == "parent" else [4.0, 4.5, 5.0]),
                   status if (which, size) == fail_at else 0))
        return [sys.executable, "-c", code]
    return command


def test_a_child_that_fails_stops_the_run(tmp_path):
    out = tmp_path / "record.txt"
    assert output_rate.run("/p", str(out), "here, today", [64, 128], command=stub(tmp_path, ("parent", 64)), limit=30) == 3
    assert (tmp_path / "started").read_text().splitlines() == ["current 64", "parent 64"]  # and nothing after it
    text = out.read_text()
    assert text.startswith(output_rate.header("here, today", [64, 128]))
    assert text.endswith("# parent at 64 ended with status 3: stopped here\n") and text.count('"a row"') == 2


def test_a_child_past_its_limit_stops_the_run(tmp_path, monkeypatch):
    """(the limit is not waited for: subprocess.run says at once what it says when a limit has run out)"""
    started = []

    def ran_out(argv, timeout, **kw):
        started.append(argv)
        raise subprocess.TimeoutExpired(argv, timeout, output="a line the child had written\n")

    monkeypatch.setattr(output_rate.subprocess, "run", ran_out)
    out = tmp_path / "record.txt"
    assert output_rate.run("/p", str(out), "here, today", [64, 128], limit=2) == 124
    assert started == [output_rate.child_command(ROOT, "current", 64)]
    assert out.read_text().endswith("a line the child had written\n# current at 64 ended with status 124: stopped here\n")


def test_a_whole_run_closes_with_the_verdicts(tmp_path):
    out = tmp_path / "record.txt"
    assert output_rate.run("/p", str(out), "here, today", [64], command=stub(tmp_path), limit=30) == 0
    assert (tmp_path / "started").read_text().splitlines() == ["current 64", "parent 64"] * 2
    last = out.read_text().splitlines()[-1]
    # the parent's six repetitions span 1 .. 3 s: the margin is 3 + 2 = 5 s, and the branch's median is 4.5 s
    assert "a row" in last and "current median 4.5 s; parent 1 .. 3 s, spread 2 s: unchanged" in last
    slow = [line("current", 64, "a row", [5.5, 6.0, 5.0]), line("parent", 64, "a row", [1.0, 3.0, 2.0])]
    assert output_rate.verdicts(slow)[0].rstrip().endswith("spread 2 s: OUTSIDE the margin")
    assert output_rate.verdicts(slow[:1]) == []  # a row one tree lacks has no verdict
