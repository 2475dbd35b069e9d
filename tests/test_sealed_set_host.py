"""The host side of sealed set decoding, without a GPU (the decode itself: tests/test_gpu_sealed_sets.py): SealError lists every failed
file, the set planner groups a sealed file by its body, and verify_set reports a file of another generation or checkpoint from its seal
alone -- a set that holds nothing else never reaches the decoder."""
import os

import pytest

import l3c_pytorch_amd  # noqa: F401
from l3c_pytorch_amd.bitcoding import container
from l3c_pytorch_amd.bitcoding.container import Seal, SealError
from l3c_pytorch_amd.helpers import dataset_codec

from tests.conftest import GOLDEN  # noqa: E402


def _golden():
    with open(os.path.join(GOLDEN, 'hip_l3c_cal_64x96.l3c'), 'rb') as f:
        return f.read()


class _NoDecoder(object):
    """Stands in for a Bitcoding where nothing may be decoded: it knows its generation and checkpoint, and nothing else."""

    def generation(self):
        return 3

    def model_id(self):
        return 0x1234


def test_seal_error_lists_every_failed_file():
    e = SealError('pixels', 2, 'x')
    assert e.index == 2 and e.failed == [2] and isinstance(e, ValueError)
    seals = [Seal(3, 10, 0), None, Seal(3, 11, 0), Seal(3, 12, 0), Seal(3, 13, 0)]
    container.check_frame_crcs(seals, [10, 99, 11, 12, 13])                       # an unsealed file's word is not compared
    with pytest.raises(SealError) as err:
        container.check_frame_crcs(seals, [10, 99, 0, 12, 7])
    assert err.value.reason == 'pixels' and err.value.index == 2 and err.value.failed == [2, 4]
    container.check_frame_crcs(seals, [10, 0, 11 - (1 << 32), 12, 13])            # int32 words as the device hands them over


def test_the_set_planner_groups_a_sealed_file_by_its_body():
    body = _golden()
    sealed = body + container.make_seal(body, 3, 0xDEADBEEF, 0x1234)
    assert container.is_sealed(sealed) and not container.is_sealed(body)
    chunks, padded = dataset_codec.plan_decode_set({'a': sealed, 'b': body, 'c': sealed}, ['a', 'b', 'c'], 16)
    assert chunks == [['a', 'b', 'c']] and padded == [(64, 96)]
    chunks, _ = dataset_codec.plan_decode_set({'a': sealed, 'b': body, 'c': sealed}, ['a', 'b', 'c'], 2)
    assert chunks == [['a', 'b'], ['c']]


def test_verify_set_reports_generation_and_model_from_the_seal_alone():
    body = _golden()
    files = {'old': body + container.make_seal(body, 2, 1, 0x1234), 'other': body + container.make_seal(body, 3, 1, 0x9999),
             'older and other': body + container.make_seal(body, 1, 1, 0x9999)}
    info = {}
    status = dataset_codec.verify_set(_NoDecoder(), files, list(files), info=info)
    assert status == {'old': 'generation', 'other': 'model', 'older and other': 'generation'} and info == {'frame_crc': {}}
    damaged = files['old'][:-1] + bytes([files['old'][-1] ^ 1])                   # a malformed seal is not a status
    with pytest.raises(ValueError, match='seal check word'):
        dataset_codec.verify_set(_NoDecoder(), {'x': damaged}, ['x'])


def test_decode_set_without_sealed_names_the_flag():
    body = _golden()
    sealed = body + container.make_seal(body, 3, 1, 0)
    with pytest.raises(ValueError, match='sealed=True.*split_seal') as e:
        dataset_codec.decode_set(_NoDecoder(), {0: sealed}, [0])
    assert not isinstance(e.value, SealError)
