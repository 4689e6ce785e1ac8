"""The store policies of ct_pvae_amd/csrc/common.h (StorePolicy; knob WT_STORES) in the gfx950 assembly -- no GPU needed
(tools/count_store_isa.py).

The helpers store_f32 / store_f32x2 compile to ONE global_store_dword / global_store_dwordx2 each -- no cache bit for the plain policy,
`sc1` for write-through, `nt` for non-temporal -- and nothing else: the three listings of a helper are equal once the bit is taken off.
The planned backward's write-through forms (rotate_bwd_planned_kernel_wt<...>, the few-angle SHORT instantiations: the ones the rule
keeps) carry `sc1` on every global store; their plain twins carry no cache bit on any; a pair of twins is the same listing otherwise,
instruction for instruction, and neither uses scratch."""
import importlib.util
import os

import pytest

TOOL = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "count_store_isa.py")
spec = importlib.util.spec_from_file_location("count_store_isa", TOOL)
tool = importlib.util.module_from_spec(spec)
spec.loader.exec_module(tool)

needs_hipcc = pytest.mark.skipif(tool.base.find_hipcc() is None, reason="hipcc is not installed")
BITS = {"plain": [], "wt": ["sc1"], "nt": ["nt"]}
WT_FORMS = {"rotate_bwd_planned_kernel_wt<%s, 1, true>" % t for t in ("2, 256, 2", "2, 1024, 2", "4, 256, 1", "4, 1024, 1")}


@needs_hipcc
def test_each_helper_is_one_store_with_its_cache_bits():
    lst = tool.listings(tool.probe_assembly())
    for helper, width in (("probe_f32", "global_store_dword"), ("probe_f32x2", "global_store_dwordx2")):
        for policy, want in BITS.items():
            ins = lst["%s_%s" % (helper, policy)]
            st = tool.stores(ins)
            print(helper, policy, st)
            assert len(st) == 1 and st[0].split()[0] == width and tool.bits(st[0]) == want, (helper, policy, st)
            assert not any(i.startswith(("buffer_wbl2", "buffer_inv")) for i in ins), (helper, policy, ins)      # no fence came with it
            assert tool.without_bits(ins) == tool.without_bits(lst[helper + "_plain"]), (helper, policy)


@needs_hipcc
def test_write_through_twins_differ_from_the_plain_kernels_in_their_store_bits_alone():
    pairs = tool.twins(tool.base.assembly())
    assert {twin for _, twin, *_ in pairs} == WT_FORMS, sorted(twin for _, twin, *_ in pairs)
    for plain, twin, a, b, scratch_a, scratch_b in pairs:
        assert a is not None, plain
        print(plain, len(a), twin, len(b))
        assert tool.stores(a) and len(tool.stores(a)) == len(tool.stores(b))
        assert all(s.startswith("global_store_dword ") for s in tool.stores(a) + tool.stores(b)), (plain, tool.stores(a), tool.stores(b))
        assert all(tool.bits(s) == ["sc1"] for s in tool.stores(b)), (twin, tool.stores(b))
        assert all(tool.bits(s) == [] for s in tool.stores(a)), (plain, tool.stores(a))
        assert len(a) == len(b) and tool.without_bits(a) == tool.without_bits(b), (plain, twin)
        assert scratch_a == 0 and scratch_b == 0, (plain, scratch_a, scratch_b)
