"""CPU-only: the host side of the GPU border clip's records (mosaic_amd/csrc/tess_records.h) on a
hand-made result (tests/native/clip_records_host.cpp).  filter_records must keep exactly the records
of tasks the device finished, demote a finished task whose record cannot be read (off + n past verts,
negative off, n = 0, negative part) and drop all its records; ClippedChips::index / chip over what is
left must build chips from the valid vertices only (the others are NaN in the input)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pts(off, n):
    return " ".join(f"{float(v):.1f} {-float(v) - 0.5:.1f}" for v in range(off, off + n))


def test_clip_record_filter_and_index(tmp_path):
    exe = tmp_path / "clip_records"
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "mosaic_amd", "csrc"), "-o", str(exe),
                    os.path.join(ROOT, "tests", "native", "clip_records_host.cpp")], check=True)
    res = subprocess.run([str(exe)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    lines = res.stdout.splitlines()
    # tasks 3, 7, 10, 12, 20, 25, 28, 30: 10 went to the host on the device; 12 (off + n past verts),
    # 20 (negative off, off + n overflowing), 28 (negative part) and 30 (n = 0) are demoted
    assert lines[0] == "demoted 4"
    assert lines[1] == "status 0 2 1 1 1 0 1 1"
    assert [ln for ln in lines if ln.startswith("ring ")] == [
        "ring 3 0 0 0 5", "ring 3 0 1 5 4", "ring 3 1 0 9 4", "ring 7 0 0 13 7", "ring 25 0 0 28 4",
        "ring 25 1 0 36 4"]
    assert [ln for ln in lines if ln.startswith("part ")] == [
        "part 3 0 1", "part 3 1 1", "part 7 0 1", "part 25 0 1", "part 25 1 1"]
    chips = [ln for ln in lines if ln.startswith("chip ")]
    assert chips == [
        f"chip 3 cell 0: b0 u6 u2 b0 u3 u2 u5 {_pts(0, 5)} u4 {_pts(5, 4)} b0 u3 u1 u4 {_pts(9, 4)}",
        f"chip 7 cell 1: b0 u3 u1 u7 {_pts(13, 7)}",
        f"chip 25 cell 0: b0 u6 u2 b0 u3 u1 u4 {_pts(28, 4)} b0 u3 u1 u4 {_pts(36, 4)}"]
    assert "nan" not in res.stdout
