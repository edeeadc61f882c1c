"""PBD_CONV_MFMA_F64 is a T = double mode: pbd_create refuses it for a float handle before it looks for a device, so this
runs with or without a GPU."""
import pytest

from partsbaseddetector_amd import model as M


def test_mode_constant_and_float_handle_refusal():
    from partsbaseddetector_amd import _lib, build, detector
    from partsbaseddetector_amd._lib import PbdError
    build.build_hip()
    assert _lib.CONV_MFMA_F64 == 4
    flat = M.synthetic_tiny_model().flatten()
    with pytest.raises(PbdError) as e:
        detector.Handle(flat, device=0, real_type=_lib.REAL_F32, conv_mode=_lib.CONV_MFMA_F64)
    assert e.value.code == -2 and "PBD_CONV_MFMA_F64 needs PBD_REAL_F64" in str(e.value)
