"""tests/helpers/batch_position.py pinned on the CPU: the arrangements are permutations that move problem 0, take / put_back
are inverse on every tensor shape the batched calls use, and first_difference finds a planted one-bit difference and says
where the problem sits in both layouts."""
import numpy as np
import pytest

from helpers import batch_position as bp

torch = pytest.importorskip("torch")

B, NX, NP, N, DIM = 77, 6, 9, 40, 70
SHAPES = [(NX, B), (NP, B), (B,), (N, B), (N, NX, B), (DIM, B), (N, NX, B)]   # the last: [n_rows, nx, B]


def _tensor(shape, dtype, seed=0):
    g = torch.Generator().manual_seed(seed)
    if dtype in (torch.int32, torch.int64):
        return torch.randint(-1000, 1000, shape, generator=g, dtype=dtype)
    return torch.randn(shape, generator=g, dtype=dtype)


@pytest.mark.parametrize("batch", [1, 2, 13, 77, 128])
def test_the_three_arrangements_are_permutations_that_move_problem_0(batch):
    for seed in range(20):
        perms = bp.permutations(batch, seed)
        assert sorted(perms) == ["reverse", "rotate1", "shuffle"]
        for name, idx in perms.items():
            assert idx.dtype == np.int64 and idx.shape == (batch,)
            assert np.array_equal(np.sort(idx), np.arange(batch)), name
            if batch > 1:
                assert idx[0] != 0, (name, seed)            # problem 0 is not at position 0 any more
        assert np.array_equal(perms["shuffle"], bp.permutations(batch, seed)["shuffle"])   # seeded: repeatable
    perms = bp.permutations(5, 3)
    assert perms["reverse"].tolist() == [4, 3, 2, 1, 0]      # problem p sits at 4 - p
    assert perms["rotate1"].tolist() == [4, 0, 1, 2, 3]      # problem p sits at p + 1, the last one first


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64, torch.int32])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_take_and_put_back_round_trip(shape, dtype):
    t = _tensor(shape, dtype)
    for name, idx in bp.permutations(B, 11).items():
        arranged = bp.take(t, idx)
        assert arranged.is_contiguous() and arranged.shape == t.shape and arranged.dtype == t.dtype
        for j in (0, 1, B - 1):
            assert torch.equal(arranged[..., j], t[..., idx[j]]), name
        back = bp.put_back(arranged, idx)
        assert back.is_contiguous() and torch.equal(back, t), name
        assert not torch.equal(arranged, t)
    for prefix in (1, 13):
        head = bp.take(t, np.arange(prefix))
        assert head.is_contiguous() and torch.equal(head, t[..., :prefix])
    with pytest.raises(ValueError):
        bp.put_back(bp.take(t, np.arange(13)), np.arange(13) + 1)
    with pytest.raises(ValueError):
        bp.put_back(t, np.arange(13))


def test_layout_of_a_position():
    assert bp.layout(0, 4) == (0, 0, 0)
    assert bp.layout(17, 4) == (1, 1, 4)         # 16 problems per wave
    assert bp.layout(76, 16) == (19, 0, 0)       # 4 per wave: 19 full waves, then one problem
    assert bp.layout(13, 5) == (1, 1, 5)         # 12 per wave, 4 riding lanes
    assert bp.layout(76, 1) == (1, 12, 12)       # one lane per problem


@pytest.mark.parametrize("dtype,bit", [(torch.float32, 0), (torch.float64, 0), (torch.float32, 3), (torch.int32, 0)])
def test_first_difference_finds_a_planted_bit(dtype, bit):
    t = _tensor((N, NX, B), dtype, seed=5)
    assert bp.first_difference(t, t.clone(), 4) is None
    idx = bp.permutations(B, 11)["reverse"]
    other = t.clone()
    itype = {torch.float32: torch.int32, torch.float64: torch.int64, torch.int32: torch.int32}[dtype]
    other.view(itype)[7, 2, 50] ^= (1 << bit)    # problem 50, entry (7, 2)
    other.view(itype)[9, 1, 60] ^= 1             # a later problem: not the first
    msg = bp.first_difference(t, other, 4, idx=idx, name="predicted_states")
    assert msg is not None and msg.startswith("predicted_states: problem 50 differs (2 of 77 problems do)"), msg
    # natural: problem 50 of 16 per wave -> wave 3, group 2, lane 8; reversed it sits at 26 -> wave 1, group 10, lane 40
    assert "natural layout (wave, group, first lane) = (3, 2, 8)" in msg, msg
    assert "arranged at position 26 = (1, 10, 40), L = 4" in msg, msg
    assert "first differing entry (7, 2, 50)" in msg, msg
    assert msg.endswith("%d ulps" % (1 << bit)), msg
    va, vb = t[7, 2, 50].item(), other[7, 2, 50].item()
    assert ("%r" % va if dtype != torch.int32 else "%d" % va) in msg and ("%r" % vb if dtype != torch.int32 else "%d" % vb) in msg
    # without an arrangement (another handle, natural order) both layouts are the natural one
    assert "arranged at position 50 = (3, 2, 8)" in bp.first_difference(t, other, 4)
    # a prefix compared with the head of the reference
    assert bp.first_difference(t[..., :13], other[..., :13], 4, idx=np.arange(13)) is None


def test_the_gpu_case_list_names_every_fused_specialisation():
    """Every (L, SP) pair and every run-time-spacing interval count that launch_fused (csrc/engine_impl.hpp) can reach -- the
    two lists of csrc/kernel_shapes.hpp it dispatches over -- is a 4-state shape of tests/test_gpu_position_independence.py:
    a specialisation added there without a case here fails this."""
    import os
    import re

    import test_gpu_position_independence as cases
    from conftest import ROOT

    with open(os.path.join(ROOT, "cart-pole-mpc_amd", "csrc", "kernel_shapes.hpp")) as fh:
        src = fh.read()
    pairs = re.search(r"using FusedStaticPairs = FusedPairList<(.*?)>;", src, re.S).group(1)
    compiled = {(int(m.group(1)), int(m.group(2))) for m in re.finditer(r"FusedPair<(\d+), (\d+)>", pairs)}
    groups = re.search(r"using FusedDynamicGroups = std::integer_sequence<int,([\d, ]*)>;", src).group(1)
    dynamic = {int(v) for v in groups.split(",")}
    assert len(compiled) >= 7 and len(dynamic) >= 6, (compiled, dynamic)   # the patterns still find the two lists
    shapes = {(N // sp, sp) for N, sp in cases.FUSED_SHAPES["single"]}
    assert all(N % sp == 0 for N, sp in cases.FUSED_SHAPES["single"] + cases.FUSED_SHAPES["double"])
    assert compiled <= shapes, compiled - shapes
    assert dynamic <= {L for L, sp in shapes - compiled}, dynamic
    assert {(N // sp, sp) for N, sp in cases.FUSED_SHAPES["double"]} <= compiled
    assert len(cases.FORMS) == 5 and len(cases.SPLIT_FORMS) == 3


def test_first_difference_compares_bit_patterns():
    nan = torch.tensor([[1.0, float("nan"), 0.0]])
    assert bp.first_difference(nan, nan.clone(), 2) is None                 # a NaN equals itself
    neg0 = torch.tensor([[1.0, float("nan"), -0.0]])
    msg = bp.first_difference(nan, neg0, 2)
    assert msg is not None and "problem 2 differs" in msg and "0 ulps" in msg, msg   # -0 is not +0, though no ulp apart
    v = torch.tensor([1.0, -1.0], dtype=torch.float64)
    w = torch.tensor([np.nextafter(1.0, 2.0), np.nextafter(np.nextafter(-1.0, -2.0), -2.0)], dtype=torch.float64)
    assert bp.first_difference(v, w, 1).endswith(" 1 ulps")
    assert bp.first_difference(v[1:], w[1:], 1).endswith(" 2 ulps")
    tiny = torch.tensor([np.float32(1e-45)])
    assert bp.first_difference(tiny, -tiny, 1).endswith(" 2 ulps")          # across zero on the ordered line
    assert "shapes / dtypes differ" in bp.first_difference(v, v.float(), 1)
