"""The guard of tests/guarded_alloc.py itself, on CPU tensors: what it returns is what torch returns (dtype, shape, strides, values),
`empty` bodies hold the poison, other devices and other functions pass through, entering, nesting and leaving change nothing of
torch, and one byte written before or after a body (through the arena: memory the guard owns) is reported with its call site.
The last test checks what can be checked of tests/contract_cases.py's table without a GPU."""
import inspect

import pytest
import torch

import guarded_alloc as ga
from guarded_alloc import GuardedAlloc

CPU = torch.device("cpu")
SHAPES = [(), (0,), (1,), (7,), (3, 5), (2, 0, 3), (4, 1, 3)]
DTYPES = [torch.float32, torch.float64, torch.int64, torch.int32, torch.uint8, torch.bool, torch.float16]


def _fill_for(dtype):
    return True if dtype == torch.bool else (3 if not dtype.is_floating_point else 2.5)


def _calls(shape, dtype):
    """(name, is it an `empty` form, thunk) for every intercepted factory at this shape and dtype."""
    like = torch.arange(max(1, int(torch.Size(shape).numel())), dtype=torch.float64)[:torch.Size(shape).numel()].reshape(shape).to(dtype)
    base = torch.ones(2, dtype=torch.int16)
    v = _fill_for(dtype)
    return [
        ("empty", True, lambda: torch.empty(shape, dtype=dtype)),
        ("empty*", True, lambda: torch.empty(*shape, dtype=dtype) if shape else torch.empty((), dtype=dtype)),
        ("zeros", False, lambda: torch.zeros(shape, dtype=dtype)),
        ("ones", False, lambda: torch.ones(shape, dtype=dtype, device="cpu")),
        ("full", False, lambda: torch.full(shape, v, dtype=dtype)),
        ("full kw", False, lambda: torch.full(shape, fill_value=v, dtype=dtype)),
        ("empty_like", True, lambda: torch.empty_like(like)),
        ("zeros_like", False, lambda: torch.zeros_like(like)),
        ("ones_like", False, lambda: torch.ones_like(like)),
        ("full_like", False, lambda: torch.full_like(like, v)),
        ("empty_like dtype", True, lambda: torch.empty_like(base, dtype=dtype).new_empty(shape)),
        ("new_empty", True, lambda: base.new_empty(shape, dtype=dtype)),
        ("new_zeros", False, lambda: base.new_zeros(shape, dtype=dtype)),
        ("new_ones", False, lambda: base.new_ones(shape, dtype=dtype)),
        ("new_full", False, lambda: base.new_full(shape, v, dtype=dtype)),
    ]


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[1])
def test_fidelity_and_poison(dtype):
    for shape in SHAPES:
        for (name, is_empty, thunk) in _calls(shape, dtype):
            want = thunk()
            with GuardedAlloc(CPU, poison=0xFF) as g:
                got = thunk()
            what = (name, shape, dtype)
            assert len(g.arenas) >= 1, what
            assert got.dtype == want.dtype and got.shape == want.shape and got.stride() == want.stride(), what
            assert got.device == want.device and got.is_contiguous() == want.is_contiguous(), what
            a = g.arenas[-1]
            assert a.nbytes == want.numel() * want.element_size(), what
            assert a.buf.numel() == ga.FRONT + a.nbytes + ga.BACK and ga.FRONT % 512 == 0, what
            if a.nbytes:   # (an empty tensor reports no address)
                assert got.data_ptr() == a.buf.data_ptr() + ga.FRONT, what
            body = a.buf[ga.FRONT:ga.FRONT + a.nbytes]
            if is_empty:
                assert bool((body == 0xFF).all()), what
            else:
                assert torch.equal(got, want), what
            assert g.violations() == [], what


def test_inferred_dtypes_and_defaults():
    with GuardedAlloc(CPU) as g:
        assert torch.full((3,), 7).dtype == torch.int64 and torch.full((3,), 7.0).dtype == torch.float32
        assert torch.full((3,), True).dtype == torch.bool
        assert torch.zeros(2, 3).dtype == torch.float32 and torch.zeros(2, 3).shape == (2, 3)
        assert torch.empty(size=(2, 5)).shape == (2, 5)
        t = torch.zeros(3, requires_grad=True)
        assert t.requires_grad and t.is_leaf
        src = torch.ones(4, 6).t()   # preserve_format: a dense non-contiguous input keeps its strides
        assert torch.empty_like(src).stride() == src.stride()
        assert torch.zeros_like(src, memory_format=torch.contiguous_format).is_contiguous()
    assert len(g.arenas) == 10 and g.violations() == []


def test_poison_zero_and_float_view():
    with GuardedAlloc(CPU, poison=0x00):
        assert bool((torch.empty(17, dtype=torch.float32) == 0).all())
    with GuardedAlloc(CPU, poison=0xFF):
        assert bool(torch.isnan(torch.empty(17, dtype=torch.float32)).all())
        assert bool((torch.empty(17, dtype=torch.int32) == -1).all())


def test_inside_autograd_function():
    class F(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x):
            out = torch.empty(x.shape, dtype=x.dtype)
            out.copy_(x * 2)
            return out

        @staticmethod
        def backward(ctx, g):
            return g.new_zeros(g.shape) + 2 * g

    x = torch.ones(5, requires_grad=True)
    with GuardedAlloc(CPU) as g:
        n0 = len(g.arenas)
        y = F.apply(x)
        assert len(g.arenas) == n0 + 1
        y.sum().backward()
    # (backward nodes run outside the mode, on the autograd engine's threads for a GPU: what they allocate is not guarded, which is
    # why the contract cases call the backward ops directly)
    assert torch.equal(x.grad, torch.full((5,), 2.0))


def test_pass_through_other_device_and_other_functions():
    with GuardedAlloc(CPU) as g:
        m = torch.empty(5, device="meta")
        torch.zeros_like(m)
        m.new_ones(3)
        assert len(g.arenas) == 0 and m.device.type == "meta"
        torch.arange(5) + 1
        torch.tensor([1.0, 2.0]).clone()
        assert len(g.arenas) == 0
        torch.empty_like(m, device="cpu")
        assert len(g.arenas) == 1
    with GuardedAlloc("meta") as g:
        torch.empty(5)
        assert len(g.arenas) == 0


def test_nesting_and_exit_leave_torch_as_it_was():
    from torch.overrides import _get_current_function_mode_stack as stack
    before = list(stack())
    funcs = (torch.empty, torch.zeros, torch.ones, torch.full, torch.empty_like, torch.Tensor.new_empty)
    with GuardedAlloc(CPU, poison=0xFF) as outer:
        with GuardedAlloc(CPU, poison=0x00) as inner:
            t = torch.empty(4, dtype=torch.int32)
            assert bool((t == 0).all())
            assert len(inner.arenas) == 1 and len(outer.arenas) == 0   # the innermost guard answers, once
        t = torch.empty(4, dtype=torch.int32)
        assert bool((t == -1).all()) and len(outer.arenas) == 1
        with pytest.raises(ZeroDivisionError):
            with GuardedAlloc(CPU):
                1 / 0
        assert list(stack())[-1] is outer
    assert list(stack()) == before
    assert funcs == (torch.empty, torch.zeros, torch.ones, torch.full, torch.empty_like, torch.Tensor.new_empty)
    t = torch.empty(1 << 12, dtype=torch.uint8)   # unguarded again: no arena grows
    assert len(outer.arenas) == 1 and t.untyped_storage().nbytes() == 1 << 12


def _line():
    return inspect.currentframe().f_back.f_lineno


@pytest.mark.parametrize("nbytes", [0, 1, 5, 512, 4099])
def test_detection_before_and_after(nbytes):
    with GuardedAlloc(CPU) as g:
        quiet = torch.empty(9)
        a = torch.empty(nbytes, dtype=torch.uint8); line_a = _line()   # noqa: E702
        b = torch.zeros(nbytes, dtype=torch.uint8); line_b = _line()   # noqa: E702
        c = torch.empty(3, dtype=torch.float32); line_c = _line()      # noqa: E702
        assert g.violations() == []
        ia, ib = g.owns(a), g.owns(b)
        assert ia is not None and ib is not None and ia != ib and g.owns(quiet) == 0 and g.owns(torch.arange(3)) is None
        g.arenas[ia].buf[ga.FRONT - 1] = 0          # one byte before the body
        g.arenas[ib].buf[ga.FRONT + nbytes] = 0     # the first byte after it
        c.as_strided((4,), (1,))[3] = 1.0           # one element past the end, the way a kernel would
        v = {x.index: x for x in g.violations()}
    assert sorted(v) == [ia, ib, g.owns(c)]
    assert v[ia].offsets == [-1] and v[ia].nbytes == nbytes and v[ia].site == (__file__, line_a)
    assert v[ib].offsets == [nbytes] and v[ib].site == (__file__, line_b)
    vc = v[g.owns(c)]
    assert vc.site == (__file__, line_c) and vc.nbytes == 12 and set(vc.offsets) <= {12, 13, 14, 15} and vc.offsets
    assert "canary" in repr(vc) and str(line_c) in repr(vc)


def test_last_byte_of_each_band_is_watched():
    with GuardedAlloc(CPU) as g:
        torch.empty(3, dtype=torch.uint8)
        buf = g.arenas[0].buf
        buf[0] = 1
        buf[-1] = 1
        (v,) = g.violations()
    assert v.offsets == [-ga.FRONT, 3 + ga.BACK - 1]


def test_the_contract_case_table_without_a_gpu():
    """Unique names; every case's decoys have its inputs' keys, shapes and dtypes and other values (Case.decoys asserts it); the
    shapes the table promises are there; NOT_DRIVEN keeps to its cap, gives reasons and names nothing of the map layer."""
    import contract_cases as cc
    from trajectory_optimization_amd import _lib
    names = [c.name for c in cc.CASES]
    assert len(set(names)) == len(names) and len(names) >= 50
    for c in cc.CASES:
        assert c.inputs and c.decoys.keys() == c.inputs.keys(), c.name
        assert not c.undefined and not c.loose, c.name   # (both empty today: a new entry needs its line and its bar, see the docstring)
    by = {c.name: c for c in cc.CASES}
    assert by["traj_plain"].inputs["points"].shape == (2049 + 37, 3) and by["traj_plain"].inputs["poses"].shape == (5, 3)
    assert by["packed_cloud_of_one_point"].inputs["points"].shape == (1, 3)
    assert by["occupancy_37_5_20"].inputs["positions"].shape == (259, 3) and by["occupancy_1_1_1"].inputs["positions"].shape == (1, 3)
    assert by["view_volume_and_select"].inputs["view_poses"].shape == (33, 3)
    map_layer = ("tohip_occ_", "tohip_los_", "tohip_field_", "tohip_evid_", "tohip_travel_", "tohip_components_", "tohip_view_volume",
                 "tohip_cast_", "tohip_depth_scan", "tohip_clearance_map", "tohip_assign_greedy")
    assert len(cc.NOT_DRIVEN) <= 20 and all(cc.NOT_DRIVEN.values())
    assert all(n in _lib.SIGNATURES and not n.startswith(map_layer) for n in cc.NOT_DRIVEN)
