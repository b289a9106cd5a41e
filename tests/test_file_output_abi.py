"""not gpu: the C-ABI of the file download (dt_hip_read_file_to_host, dt_hip_batch_set_file_output,
dt_hip_batch_file_bytes): exported and mirrored, refusing with a negative code where there is no device or no batch, and
DT_HIP_FILE_TOO_LARGE a code of its own in the header and in the mirror."""
import ctypes as C
import os
import re

import numpy as np

from ansel_amd import abi, lib, pipe

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_codes():
    src = open(os.path.join(ROOT, "include", "ansel_hip.h")).read()
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"#define (DT_HIP_\w+) \((-\d+)\)", src)}


def test_file_too_large_is_a_code_of_its_own():
    codes = _header_codes()
    assert codes["DT_HIP_FILE_TOO_LARGE"] == -995 == abi.DT_HIP_FILE_TOO_LARGE
    assert codes["DT_HIP_WRITER_FAILED"] == abi.DT_HIP_WRITER_FAILED
    assert len(set(codes.values())) == len(codes), codes
    others = (abi.DT_HIP_SUCCESS, abi.DT_HIP_DEFAULT_ERROR, abi.DT_HIP_SYSMEM_ALLOCATION, abi.DT_HIP_INVALID_ARG,
              abi.DT_HIP_WRITER_FAILED)
    assert abi.DT_HIP_FILE_TOO_LARGE not in others


def test_the_three_entries_are_exported_and_mirrored():
    l = lib.load()
    for name in ("dt_hip_read_file_to_host", "dt_hip_batch_set_file_output", "dt_hip_batch_file_bytes"):
        assert name in l._ansel_protos and name not in l._ansel_missing, name
    assert hasattr(pipe.DevicePipe, "read_file")


def test_without_a_device_or_a_batch_every_entry_refuses():
    """no device is initialised here (and none need exist): device 0 is no device, NULL is no batch"""
    l = lib.load()
    host = np.full(64, 0xA5, np.uint8)
    rc = l.dt_hip_read_file_to_host(0, C.c_void_p(4096), 64, host.ctypes.data, 64)
    assert rc < 0
    assert l.dt_hip_last_error()
    assert (host == 0xA5).all()
    assert l.dt_hip_read_file_to_host(-1, None, 0, None, 0) < 0
    assert l.dt_hip_batch_set_file_output(None, 64) < 0
    n = C.c_size_t(77)
    assert l.dt_hip_batch_file_bytes(None, 0, C.byref(n)) < 0
    assert n.value == 77
