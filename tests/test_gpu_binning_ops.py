"""Builds tests/hip_unit/binning_ops.hip against g4splat_amd/csrc/binning.hip with the library's own compiler flags and
runs it: every launcher of the binning stage (three radix sorts, two block-sum scans, compaction, instance expansion, tile
ranges, tile order) against host restatements, bit for bit, at the sizes where their code paths switch."""
import os
import subprocess

import pytest

from support import HIPCC, build_harness


@pytest.mark.skipif(HIPCC is None, reason="hipcc not installed")
def test_binning_harness_compiles_and_links(tmp_path):
    """No GPU needed: a signature change in g4s_internal.h, or a launcher that binning.hip stops exporting, breaks here."""
    assert os.path.getsize(build_harness(tmp_path, "binning_ops", "binning.hip")) > 0


@pytest.mark.gpu
def test_binning_kernels_against_host_restatements(tmp_path):
    exe = build_harness(tmp_path, "binning_ops", "binning.hip")
    res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    print(res.stdout[-6000:])
    assert res.returncode == 0 and "binning_ops OK" in res.stdout, res.stdout[-20000:]
