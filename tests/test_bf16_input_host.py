"""Host-side behaviour of dense bfloat16 input (corrla_rs_amd/api.py), no GPU needed: the normaliser keeps a bf16 tensor
instead of widening it, the symbol suffix, and the surfaces without a bf16 entry refuse one before touching the library."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from corrla_rs_amd import _lib as L
from corrla_rs_amd import api


def test_as_dense_keeps_a_cpu_bf16_tensor():
    t = torch.arange(12, dtype=torch.float32).reshape(4, 3).to(torch.bfloat16)
    a, on_dev = api._as_dense(t, "a_mat")
    assert a.dtype == torch.bfloat16 and not on_dev
    assert a.data_ptr() == t.data_ptr()          # kept as it is: no copy, no widening
    assert api._strides(a) == (3, 1) and api._strides(api._as_dense(t.t(), "a_mat")[0]) == (1, 3)
    with pytest.raises(ValueError):
        api._as_dense(torch.zeros(5, dtype=torch.bfloat16), "a_mat")


def test_every_other_dtype_keeps_todays_rule():
    a, on_dev = api._as_dense(torch.zeros((4, 3), dtype=torch.float16), "a_mat")
    assert isinstance(a, np.ndarray) and a.dtype == np.float64 and not on_dev
    a, _ = api._as_dense(torch.zeros((4, 3), dtype=torch.float32), "a_mat")
    assert isinstance(a, np.ndarray) and a.dtype == np.float32
    a, _ = api._as_dense(np.zeros((4, 3), dtype=np.int32), "a_mat")
    assert a.dtype == np.float64


def test_suffix_knows_bf16():
    assert api._suffix(torch.bfloat16) == "bf16"
    assert api._suffix(torch.float32) == "f32" and api._suffix(np.dtype(np.float32)) == "f32"
    assert api._suffix(torch.float64) == "f64" and api._suffix(np.dtype(np.float64)) == "f64"


def test_bf16_entries_are_bound_like_their_f32_twins():
    for name in ("corrla_rsvd_", "corrla_rsvd_dev_", "corrla_pca_", "corrla_pca_dev_", "corrla_matmul_dev_"):
        assert L.SIGNATURES[name + "bf16"] == L.SIGNATURES[name + "f32"]
    assert "n_bf16_products" in [f for f, _ in L.Timings._fields_]
    for absent in ("corrla_rsvd_sharded_dev_bf16", "corrla_pca_sharded_dev_bf16", "corrla_power_iter_bf16"):
        assert absent not in L.SIGNATURES


def test_outputs_of_a_bf16_call_are_modelled_on_float32():
    like = api._f32_like(torch.zeros((2, 2), dtype=torch.bfloat16))
    assert isinstance(like, np.ndarray) and like.dtype == np.float32
    out = api._empty_colmajor(like, 5, 3)
    assert out.dtype == np.float32 and out.flags.f_contiguous


class _NoLibrary:
    """stands where the loaded library would be: any use of it fails the test"""

    def __getattr__(self, name):
        raise AssertionError(f"the library was touched ({name})")


@pytest.fixture
def ctx():
    c = api.Context.__new__(api.Context)   # no device, no library
    c._lib, c._h, c.device = _NoLibrary(), None, 0
    return c


def test_surfaces_without_a_bf16_entry_raise_before_touching_the_library(ctx):
    t = torch.zeros((8, 4), dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="bfloat16"):
        ctx.rsvd_sharded(t, 2, 1, 1)
    with pytest.raises(ValueError, match="bfloat16"):
        ctx.rsvd_sharded(t, 2, 1, 1, shard="cols")
    with pytest.raises(ValueError, match="bfloat16"):
        ctx.pca_sharded(t, 2)
    with pytest.raises(ValueError, match="bfloat16"):
        ctx.power_iter(t, 2, 1)
    with pytest.raises(ValueError, match="bfloat16"):
        api.power_iter(t, 2, 1, ctx=ctx)


def test_matmul_refuses_a_bf16_skinny_operand_before_touching_the_library(ctx):
    a = torch.zeros((8, 4), dtype=torch.bfloat16)
    with pytest.raises(ValueError):
        ctx.matmul(a, torch.zeros((4, 2), dtype=torch.bfloat16))
    with pytest.raises(ValueError):
        ctx.matmul(torch.zeros((8, 4)), torch.zeros((4, 2), dtype=torch.bfloat16))
    with pytest.raises(ValueError):
        ctx.matmul(a, torch.zeros((4, 2), dtype=torch.float64))
