"""Builds tests/hip_unit/scan_ops.hip against g4splat_amd/csrc/tsdf/scan.hip alone, with the library's own compiler
flags, and runs it: scan_u32 against a host loop, bit for bit, for n = 0, 1, 255, 1023, 1024, 1025, 262144 (256 chunks)
and 262145 (257 chunks: the second trip of scan_chunk_offs_kernel's loop), on seeded values in 0..7 and on all ones."""
import os
import shutil
import subprocess

import pytest

from support import HIPCC, build_harness


@pytest.mark.skipif(HIPCC is None, reason="hipcc not installed")
def test_scan_harness_compiles_and_links(tmp_path):
    """No GPU needed: scan.hip must stand on its own -- a dependency on another translation unit breaks the link here."""
    assert os.path.getsize(build_harness(tmp_path, "scan_ops", "tsdf/scan.hip")) > 0


@pytest.mark.gpu
def test_scan_u32_against_a_host_loop(tmp_path):
    exe = build_harness(tmp_path, "scan_ops", "tsdf/scan.hip")
    for kind in ("seeded", "ones"):  # one program run each, under its own time limit; nothing runs after a failure
        res = subprocess.run([shutil.which("timeout"), "-k", "10", "60", exe, kind], stdout=subprocess.PIPE,
                             stderr=subprocess.STDOUT, text=True)
        print(res.stdout[-4000:])
        assert res.returncode == 0 and f"scan_ops OK {kind}" in res.stdout, (kind, res.returncode, res.stdout[-8000:])
