"""CPU suite: wide graphs (lists of up to 128 ids — HNSW graph_degree <= 64, i.e. M0 = 2 M <= 128; DiskANN R <= 128) pass every
validation layer, and one id more is refused with the range in the message.  A well-formed wide graph gets as far as the device
(LEANN_ERR_DEVICE on a box without a GPU).  No GPU needed."""
import struct

import numpy as np
import pytest

from util import synth, write_gx1


@pytest.fixture(scope="module")
def wide(po):
    X = synth(po, 3000, 128)
    G = po.Graph.build_hnsw(X, M=64, efc=128)
    lv, uo, a0, aU = G.export()
    assert a0.shape[1] == 128 and (a0[:, 64:] != 0xFFFFFFFF).any()  # some level-0 lists really hold more than 64 ids
    return dict(X=X, M=64, M0=128, max_level=G.max_level, entry=G.entry, levels=lv, upper_off=uo, adj0=a0, adjU=aU)


def _open(la, tmp_path):
    return la.BackendSearcher.load(0, str(tmp_path / "documents.leann"), 128)


def test_wide_index_file_reaches_the_device(la, wide, tmp_path):
    write_gx1(tmp_path / "documents.index", 0, **wide)
    if la.device_count() > 0:
        s = _open(la, tmp_path)
        assert s.len() == 3000 and s.graph_info()["M0"] == 128
        s.close()
    else:
        with pytest.raises(la.LeannError) as e:
            _open(la, tmp_path)
        assert e.value.code == 4 and "no CPU fallback" in str(e.value)  # validation passed; only the GPU is missing


@pytest.mark.parametrize("field,off", [("M0", 32), ("M", 28)])
def test_129_ids_per_list_is_out_of_range(la, wide, tmp_path, field, off):
    write_gx1(tmp_path / "documents.index", 0, **wide)
    raw = bytearray((tmp_path / "documents.index").read_bytes())
    struct.pack_into("<I", raw, off, 129)
    (tmp_path / "documents.index").write_bytes(bytes(raw))
    with pytest.raises(la.LeannError) as e:
        _open(la, tmp_path)
    assert e.value.code == 3 and "out of range" in str(e.value), str(e.value)


def test_from_arrays_accepts_128_ids(la, wide):
    args = (wide["X"], 64, 128, wide["max_level"], wide["entry"], wide["levels"], wide["upper_off"], wide["adj0"], wide["adjU"])
    if la.device_count() > 0:
        la.BackendSearcher.from_arrays(la.BackendType.Hnsw, *args).close()
    else:
        with pytest.raises(la.LeannError) as e:
            la.BackendSearcher.from_arrays(la.BackendType.Hnsw, *args)
        assert e.value.code == 4


def test_from_arrays_refuses_129_ids(la, wide):
    a0 = np.concatenate([wide["adj0"], np.full((3000, 1), 0xFFFFFFFF, np.uint32)], axis=1)
    with pytest.raises(la.LeannError) as e:
        la.BackendSearcher.from_arrays(la.BackendType.Hnsw, wide["X"], 64, 129, wide["max_level"], wide["entry"], wide["levels"],
                                       wide["upper_off"], a0, wide["adjU"])
    assert e.value.code == 3 and "[1, 128]" in str(e.value)


@pytest.mark.parametrize("backend,degree,rng", [(0, 65, "[2, 64]"), (1, 129, "[2, 128]"), (0, 1, "[2, 64]"), (1, 1, "[2, 128]")])
def test_build_refuses_degrees_past_the_range(la, tmp_path, backend, degree, rng):
    X = np.zeros((4, 8), np.float32)
    with pytest.raises(la.LeannError) as e:
        la.BackendBuilder(la.BackendType(backend)).build(X, [], str(tmp_path / "documents.leann"), 8, degree, 32)
    assert e.value.code == 1 and rng in str(e.value), str(e.value)  # LEANN_ERR_INVALID, before any device work


@pytest.mark.parametrize("backend,degree", [(0, 64), (1, 128)])
def test_build_accepts_the_widest_degrees(la, tmp_path, backend, degree):
    if la.device_count() > 0:
        pytest.skip("covered on the GPU by tests/test_gpu_wide_degree.py")
    X = np.zeros((4, 8), np.float32)
    with pytest.raises(la.LeannError) as e:
        la.BackendBuilder(la.BackendType(backend)).build(X, [], str(tmp_path / "documents.leann"), 8, degree, 32)
    assert e.value.code == 4 and "no CPU fallback" in str(e.value)  # the degree passed; only the GPU is missing


def test_device_build_refuses_degrees_past_the_range(la):
    X = np.zeros((4, 8), np.float32)
    for backend, degree, rng in ((0, 65, "[2, 64]"), (1, 129, "[2, 128]")):
        with pytest.raises(la.LeannError) as e:
            la.BackendSearcher.build_device(la.BackendType(backend), X.ctypes.data, 4, 8, 8, degree, 32)
        assert e.value.code == 1 and rng in str(e.value), str(e.value)
