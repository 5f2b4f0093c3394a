"""The streaming tier's group (include/dvda_mlp_hip.h, tier B: dvda_hip_open_mlpdecoder_group ...) where no GPU is needed:
the symbols, the binding, the answers on a NULL handle, and that there is no CPU fallback behind the open."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("dvda_hip_open_mlpdecoder_group", "dvda_hip_close_mlpdecoder_group", "dvda_hip_mlpdecoder_group_size",
           "dvda_hip_mlpdecoder_group_decode_packets", "dvda_hip_mlpdecoder_group_status",
           "dvda_hip_mlpdecoder_group_queued_bytes", "dvda_hip_mlpdecoder_group_path", "dvda_hip_mlpdecoder_group_steps")


def test_library_exports_and_binding(pkg):
    hip = pkg.hipdec
    L = hip.lib()
    header = open(os.path.join(ROOT, "include", "dvda_mlp_hip.h")).read()
    for name in SYMBOLS:
        assert hasattr(L, name), name
        assert name in hip.EXPORTS, name
        assert re.search(r"\b%s\(" % name, header), name
        assert getattr(L, name).argtypes is not None, name          # bound with its signature, not by default
    assert int(re.search(r"#define DVDA_STREAM_GROUP_MAX (\d+)u", header).group(1)) == hip.STREAM_GROUP_MAX == 256
    step = open(os.path.join(ROOT, "libdvd-audio_amd", "csrc", "mlp_step.h")).read()
    assert int(re.search(r"#define DVDA_STEP_MAX_MEMBERS (\d+)u", step).group(1)) == hip.STREAM_GROUP_MAX
    assert callable(hip.MLPDecoderGroup)


def _no_such_device():
    """a device index nothing answers to: 0 on a machine without a GPU, one past the last elsewhere"""
    import torch
    return torch.cuda.device_count() if torch.cuda.is_available() else 0


def test_no_cpu_fallback_without_a_device(pkg):
    """Where there is no HIP device to open the group on, the open returns NULL and the class raises: nothing decodes on
    the CPU.  (On a machine with GPUs the device asked for is one that does not exist.)"""
    hip = pkg.hipdec
    dev = _no_such_device()
    for n in (1, 8):
        assert not hip.lib().dvda_hip_open_mlpdecoder_group(n, dev)
    with pytest.raises(hip.HipError, match="no CPU fallback"):
        hip.MLPDecoderGroup(4, device=dev)
    # out of range: refused before any device is looked at
    for n in (0, hip.STREAM_GROUP_MAX + 1):
        assert not hip.lib().dvda_hip_open_mlpdecoder_group(n, dev)
        with pytest.raises(hip.HipError):
            hip.MLPDecoderGroup(n, device=dev)


def test_null_handle(pkg):
    """as the lone decoder's accessors: all-ones / 0 / -1"""
    L = pkg.hipdec.lib()
    assert L.dvda_hip_mlpdecoder_status(None) == 0xFFFFFFFF        # (the lone ones, for comparison)
    assert L.dvda_hip_mlpdecoder_group_status(None, 0) == 0xFFFFFFFF
    assert L.dvda_hip_mlpdecoder_group_queued_bytes(None, 0) == 0
    assert L.dvda_hip_mlpdecoder_group_path(None, 0) == -1
    assert L.dvda_hip_mlpdecoder_group_size(None) == 0
    assert L.dvda_hip_mlpdecoder_group_steps(None) == 0
    frames = (ctypes.c_uint * 1)(7)
    assert L.dvda_hip_mlpdecoder_group_decode_packets(None, None, None, frames, None, None) == 0
    L.dvda_hip_close_mlpdecoder_group(None)
