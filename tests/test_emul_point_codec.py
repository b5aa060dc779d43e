"""The square roots (field.h, field29.h, fp2.h) and the compressed points and proofs (csrc/pointcodec.hip) on the CPU thread emulator:
the kernel SOURCES compiled by g++ (tests/emul), every result compared with Python integers.  The checks themselves are in
tests/point_codec_common.py; tests/test_gpu_point_codec.py runs them again on the device.  Calls stay at <= 257 elements: the
emulator runs a wavefront's lanes one after the other."""
import ctypes as C

import pytest

import point_codec_common as pc
from emul_util import SO_PATH, emul_bn128


@pytest.fixture(scope="module")
def bn():
    return emul_bn128()


def _dev(data):
    """the emulator's device memory is the host's"""
    buf = (C.c_uint8 * max(len(data), 1)).from_buffer_copy(data or b"\0")
    return C.addressof(buf), buf


@pytest.mark.parametrize("impl", [0, 2])
def test_fq_roots(bn, impl):
    pc.check_fq_roots(bn, impl)


@pytest.mark.parametrize("impl", [0, 2])
def test_fq2_roots(bn, impl):
    pc.check_fq2_roots(bn, impl)


def test_fr_has_no_root(bn):
    pc.check_fr_has_no_root(bn)


def test_literal_vectors(bn):
    pc.check_literal_vectors(bn)


@pytest.mark.parametrize("g", [1, 2])
def test_codec_against_python_integers(bn, g):
    pc.check_codec(bn, g)


@pytest.mark.parametrize("g", [1, 2])
def test_planted_bad_encodings(bn, g):
    pc.check_planted_points(bn, g)


@pytest.mark.parametrize("g", [1, 2])
def test_more_than_one_chunk(bn, tune, g):
    pc.check_chunked_stream(bn, tune, g)


def test_proof_codec(bn):
    pc.check_proof_codec(bn)


def test_planted_proofs_alone_in_a_batch_and_through_device_pointers(bn):
    pc.check_planted_proofs(bn, _dev)


def test_reference_verifier_vectors_compressed(bn):
    pc.check_golden_verify_compressed(bn)


def test_golden_proofs_compressed(bn):
    pc.check_golden_proofs_compressed(bn)


def test_errors_leave_the_outputs_untouched(bn):
    pc.check_errors(bn, SO_PATH)
