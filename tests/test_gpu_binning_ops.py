"""Builds tests/hip_unit/binning_ops.hip against g4splat_amd/csrc/binning.hip with the library's own compiler flags and
runs it: every launcher of the binning stage (three radix sorts, two block-sum scans, compaction, instance expansion, tile
ranges, tile order) against host restatements, bit for bit, at the sizes where their code paths switch."""
import os
import re
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "g4splat_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else shutil.which("hipcc")


def makefile_cxxflags():
    """CXXFLAGS of g4splat_amd/csrc/Makefile, with $(ARCH) resolved from the same file."""
    text = open(os.path.join(CSRC, "Makefile")).read()
    arch = re.search(r"^ARCH\s*\?=\s*(\S+)", text, re.M).group(1)
    flags = re.search(r"^CXXFLAGS\s*=\s*(.+)$", text, re.M).group(1).replace("$(ARCH)", arch).split()
    assert "--offload-arch=gfx950" in flags and "-ffp-contract=off" in flags, flags
    return flags


def build_harness(tmp_path):
    exe = str(tmp_path / "binning_ops")
    cmd = [HIPCC] + makefile_cxxflags() + [os.path.join(HERE, "hip_unit", "binning_ops.hip"), os.path.join(CSRC, "binning.hip"),
                                           "-o", exe]
    res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert res.returncode == 0, res.stdout
    return exe


@pytest.mark.skipif(HIPCC is None, reason="hipcc not installed")
def test_binning_harness_compiles_and_links(tmp_path):
    """No GPU needed: a signature change in g4s_internal.h, or a launcher that binning.hip stops exporting, breaks here."""
    assert os.path.getsize(build_harness(tmp_path)) > 0


@pytest.mark.gpu
def test_binning_kernels_against_host_restatements(tmp_path):
    exe = build_harness(tmp_path)
    res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    print(res.stdout[-6000:])
    assert res.returncode == 0 and "binning_ops OK" in res.stdout, res.stdout[-20000:]
