"""The fused block schedule's hand-offs by name (no GPU): the argument records of edge_block.py
mirror their Functions' forward signatures, and BlockCarry takes, clears and reports its fields."""
import inspect

import pytest

from gasfm_amd import edge_block
from gasfm_amd.model import BlockCarry


@pytest.mark.parametrize("record, fn, skip", [
    (edge_block.EpilogueArgs, edge_block.EdgeEpilogueFn, 1),  # after ctx
    (edge_block.Epilogue0Args, edge_block.Block0EpilogueFn, 1),
    (edge_block.CamArgs, edge_block.EdgeCamFn, 2),  # after ctx, P
])
def test_record_fields_are_the_forward_parameters(record, fn, skip):
    """A parameter inserted into or reordered in a forward fails here, not as a wrong pointer of
    the right dtype in a kernel; trailing defaults included."""
    params = list(inspect.signature(fn.forward).parameters.values())[skip:]
    assert record._fields == tuple(p.name for p in params)
    defaults = {p.name: p.default for p in params if p.default is not inspect.Parameter.empty}
    assert record._field_defaults == defaults


def test_seam_functions_take_an_epilogue_record_then_cam_args():
    """SeamFn / Seam0Fn.apply(*epi, *cam): as many parameters as the two records have fields, the
    defaulted tail of CamArgs defaulted there as well."""
    for fn, epi in ((edge_block.SeamFn, edge_block.EpilogueArgs), (edge_block.Seam0Fn, edge_block.Epilogue0Args)):
        params = list(inspect.signature(fn.forward).parameters.values())[1:]
        assert len(params) == len(epi._fields) + len(edge_block.CamArgs._fields)
        assert [p.default for p in params[-2:]] == [edge_block.CamArgs._field_defaults[k] for k in ("P0", "dwp")]


def test_block_carry_take_clears_and_pending_lists_what_is_set():
    c = BlockCarry()
    assert c.pending() == []
    c.SA, c.XRc = "sa", "xrc"
    assert sorted(c.pending()) == ["SA", "XRc"]
    assert c.take("SA") == "sa" and c.SA is None and c.take("SA") is None
    assert c.pending() == ["XRc"]
    assert c.take("XRc") == "xrc" and c.pending() == []


def test_block_carry_rejects_unknown_names():
    c = BlockCarry()
    with pytest.raises(AttributeError):
        c.take("XRC")
    with pytest.raises(AttributeError):
        c.XRC = 1
