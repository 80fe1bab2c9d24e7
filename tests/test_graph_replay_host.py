"""CPU: the host side of tests/test_gpu_graph_replay.py (tests/graph_replay.py) -- the three tables partition the header's
stream-taking entry points, every refusal is a sentence of the header, host arrays are rewritten with other valid values of the same
type, slots refuse a value set of another shape, and the call log notes the recording state."""
import ctypes as C

import numpy as np
import pytest
import torch

import graph_replay as GR
import stream_order as SO


def test_the_three_tables_partition_the_stream_taking_entry_points():
    errors = GR.partition_errors()
    assert errors == dict(missing=[], unknown=[], twice=[]), errors
    assert len(GR.REPLAYED) + len(GR.REFUSED_WHILE_RECORDING) + len(GR.EXEMPT) == len(SO.abi_stream_functions())


def test_partition_errors_are_reported_by_name():
    names = set(SO.abi_stream_functions()) | {'rohm_new_call'}
    names.discard('rohm_gemm_f32')
    errors = GR.partition_errors(names)
    assert errors['missing'] == ['rohm_new_call'] and errors['unknown'] == ['rohm_gemm_f32'] and errors['twice'] == []


def test_every_refusal_is_a_sentence_of_the_header():
    prose = SO.header_prose()
    for name, sentence in GR.REFUSED_WHILE_RECORDING.items():
        assert sentence.startswith(name) and sentence.endswith('.'), name
        assert sentence in prose, f'{name}: the header does not say {sentence!r}'
    assert 'returns ROHM_ERR_UNSUPPORTED with a rohm_last_error that names the function, before it issues or synchronises anything' in prose
    assert 'tests/test_gpu_graph_replay.py' in prose
    # what is refused while recording is documented as waiting, and the other way round (set-up calls without a stream apart)
    waiting = {f for f in SO.SYNC_DOCUMENTED if f in SO.abi_stream_functions() and f not in SO.SYNC_ONLY_IN}
    assert waiting == set(GR.REFUSED_WHILE_RECORDING), (waiting, set(GR.REFUSED_WHILE_RECORDING))


def test_every_exemption_has_a_reason_and_every_replayed_entry_a_family():
    assert all(isinstance(r, str) and len(r) > 20 for r in GR.EXEMPT.values())      # (EXEMPT is empty today)
    assert set(GR.REPLAYED.values()) == {'ops', 'planes', 'ddpm', 'posenet', 'trajnet', 'train', 'guided', 'smplx', 'repr', 'export', 'render', 'image',
                                          'train_helpers', 'data', 'metrics', 'track', 'multiview', 'fit_views', 'rig'}


@pytest.mark.parametrize('a, lo, hi', [
    (np.asarray([400, 397, 394, 391], np.int64), 0, 999),
    (np.asarray([5, 5, 5], np.int64), 0, 99),                                  # constant: only the given range lets it differ
    (np.asarray([[0.05, 0.95, 0.1], [0.06, 0.94, 0.0]], np.float32), 0.0, 1.0),
    (np.asarray([0, 7, 0], np.int32), None, None),                              # symmetric: mirrored and reversed it is itself
    (np.arange(130, dtype=np.int64)[::-1].copy() % 100, 0, 99),
    (np.asarray([0, 255], np.uint8), None, None),
])
def test_rewrite_valid_keeps_dtype_shape_and_range_and_changes_every_element(a, lo, hi):
    before = a.copy()
    old = GR.rewrite_valid(a, lo, hi)
    assert (old == before).all() and a.dtype == before.dtype and a.shape == before.shape
    assert (a != before).all()
    assert a.min() >= (before.min() if lo is None else lo) and a.max() <= (before.max() if hi is None else hi)


def test_rewrite_valid_refuses_what_it_cannot_rewrite():
    with pytest.raises(ValueError, match='cannot differ'):
        GR.rewrite_valid(np.asarray([3, 3], np.int64))
    with pytest.raises(ValueError, match='leaves'):
        GR.rewrite_valid(np.asarray([3, 120], np.int64), 0, 99)
    with pytest.raises(ValueError, match='numpy array'):
        GR.rewrite_valid([1, 2, 3])


def test_rewrite_tables_leaves_only_in_bounds_combinations():
    bufs = [torch.zeros(n) for n in (5, 2100, 64)]
    tables = [(C.c_void_p * 3)(*[b.data_ptr() for b in bufs]) for _ in range(2)]
    numel = (C.c_longlong * 3)(5, 2100, 64)
    GR.rewrite_tables(tables, numel)
    assert list(numel) == [5, 5, 5]
    assert all(list(t) == [bufs[1].data_ptr()] * 3 for t in tables)
    with pytest.raises(ValueError):
        GR.rewrite_tables([(C.c_void_p * 1)(bufs[0].data_ptr())], (C.c_longlong * 1)(5))
    with pytest.raises(ValueError, match='length'):
        GR.rewrite_tables([(C.c_void_p * 2)()], (C.c_longlong * 3)(1, 2, 3))


def test_slots_keep_their_address_and_refuse_another_shape_or_dtype():
    s = GR.Slots('cpu')
    slot = s.add('x', torch.arange(6.0).reshape(2, 3), torch.ones(2, 3))
    t = s.add('t', torch.tensor([0, 9, 4]), torch.tensor([3, 1, 7]))
    assert torch.isnan(slot).all() and (t == 0).all()               # pre-filled: NaN for floats, a valid index for integers
    at = slot.data_ptr()
    s.load(2)
    assert torch.equal(slot, torch.ones(2, 3)) and t.tolist() == [3, 1, 7]
    s.load(1)
    assert torch.equal(s['x'], torch.arange(6.0).reshape(2, 3)) and s['x'].data_ptr() == at and t.tolist() == [0, 9, 4]
    with pytest.raises(ValueError, match='value set 2 is'):
        s.add('y', torch.zeros(2, 3), torch.zeros(3, 2))
    with pytest.raises(ValueError, match='value set 2 is'):
        s.add('z', torch.zeros(2, 3), torch.zeros(2, 3, dtype=torch.float64))
    with pytest.raises(ValueError, match='exists'):
        s.add('x', torch.zeros(1), torch.zeros(1))
    with pytest.raises(ValueError, match='two value sets'):
        s.add('w', torch.zeros(1))
    with pytest.raises(ValueError):
        s.load(3)


class _Fake:
    def rohm_fake_a(self, x, stream):
        return 0

    def rohm_fake_b(self, x, stream):
        return 0


def test_the_call_log_notes_the_recording_state_and_checks_the_claims():
    state = {'capturing': False}
    fake, log = _Fake(), GR.RecordingLog(is_capturing=lambda: state['capturing'], current_stream=lambda: 0x10)
    with log.installed(fake, {'rohm_fake_a': 1, 'rohm_fake_b': 1}):
        state['capturing'] = True
        fake.rohm_fake_a(None, 0x10)
        with pytest.raises(AssertionError, match='rohm_fake_a was handed the stream 0x20'):
            fake.rohm_fake_a(None, 0x20)
    assert log.recorded() == {'rohm_fake_a'} and log.outside() == []
    log.check_claims(['rohm_fake_a'])
    with pytest.raises(AssertionError, match=r"never called while the stream was recording: \['rohm_fake_b'\]"):
        log.check_claims(['rohm_fake_a', 'rohm_fake_b'])
    with log.installed(fake, {'rohm_fake_b': 1}):
        state['capturing'] = False
        fake.rohm_fake_b(None, 0x10)
    with pytest.raises(AssertionError, match='NOT recording'):
        log.check_claims(['rohm_fake_a'])
    assert fake.rohm_fake_a.__func__ is _Fake.rohm_fake_a            # the originals are back
