"""Host property test of ``closed_ticket`` (nano-hevc_amd/csrc/nh_closed_ticket.hpp),
the ticket -> (set, plane, block row) map both closed-loop row wavefronts claim
their rows with.  A wrong map does not give wrong
samples on the device, it gives a stall at particular shapes, so the map is
walked on the CPU: tests/closed_ticket_check.cpp includes the very header the
kernels include, is built with the oracle's host compiler under
-fsanitize=address,undefined (a stand-alone program with its own main) and run
once.  It checks, for both orders, every layout of 1..3 sets with np 0..3 and
bh 0..4, 4,000 seeded random layouts of up to 8 sets, the 64-frame 1080p YUV420
stream and the layouts of test_closed_wavefront_gpu.py: tickets map one-to-one
onto the rows, row by-1 of a plane is claimed before row by, and in order 1 the
block row never decreases with the ticket."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(ROOT, "nano-hevc_amd", "csrc")


def _oracle_cc():
    """The compiler oracle/Makefile builds with: $CC, else its ``CC ?=`` default."""
    with open(os.path.join(ROOT, "oracle", "Makefile")) as f:
        default = re.search(r"^CC \?= *(\S+)", f.read(), re.M).group(1)
    return os.environ.get("CC", default)


def test_closed_ticket_properties(tmp_path):
    exe = str(tmp_path / "closed_ticket_check")
    cmd = [_oracle_cc(), "-x", "c++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
           os.path.join(HERE, "closed_ticket_check.cpp"), "-o", exe, "-lstdc++"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout, r.stderr[-2000:])
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-2000:])
    m = re.search(r"closed_ticket ok: (\d+) layouts, (\d+) tickets", r.stdout)
    # 2 orders x (20 + 400 + 8000 exhaustive + 4000 random + 4 named) less the layouts without a row
    assert m and int(m.group(1)) > 20000 and int(m.group(2)) > 1000000, r.stdout
