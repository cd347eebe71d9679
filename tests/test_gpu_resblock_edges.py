"""Every shipped dense route of the fused ResBlock kernels (vo_resblock_pair, vo_resblock_pair_frag, vo_resblock3,
vo_resblockk) at its tile and halo edges, per element and per row against float64 with guard utterances around
x, y and acc (tests/resblock_check.py).  The tile rows come from the library (vo_resblock_pair_tile_rows,
vo_resblock3_tile_rows, vo_resblockk_tile_rows), so the edges follow a retiling.  B = 3: one utterance has
neighbours on both sides and an utterance boundary falls inside a persistent workgroup's run of tiles."""
import pytest
import torch

import resblock_check as RC

pytestmark = pytest.mark.gpu


def _tile_rows(name, entry, C, K, dils, knob):
    """The route's output rows per tile, asked of the library under the route's knob (host only: no GPU call)."""
    from visual_onoma_to_wave_amd import _lib, ops
    if knob:
        _lib.lib().vo_tune(knob[0].encode(), knob[1])
    try:
        if entry == "blockk":
            return ops.resblock_k_tile_rows(K)
        if entry == "block3":
            return ops.resblock3_tile_rows(C, dils)
        return ops.resblock_pair_tile_rows(C, K, dils[0], frag=entry == "pair_frag")
    finally:
        if knob:
            _lib.lib().vo_tune(knob[0].encode(), 0)


def _call(c, d):
    """The case's ops call on the device views; d: device tensors."""
    from visual_onoma_to_wave_amd import ops
    kw = dict(out=d["y"], out_scale=c["out_scale"], acc=d["acc"])
    if c["entry"] in ("pair", "pair_frag"):
        frag = c["entry"] == "pair_frag"
        w1, w2 = (ops.pack_frag(d["p1"][0]), ops.pack_frag(d["p2"][0])) if frag else (d["p1"][0], d["p2"][0])
        return ops.resblock_pair(d["x"], w1, d["b1"][0], w2, d["b2"][0], c["K"], c["dils"][0], c["slope"], frag=frag,
                                 **kw)
    if c["entry"] == "block3":
        return ops.resblock3(d["x"], d["p1"], d["b1"], d["p2"], d["b2"], c["dils"], c["slope"], **kw)
    return ops.resblock_k(d["x"], d["p1"], d["b1"], d["p2"], d["b2"], c["K"], c["dils"], c["slope"], **kw)


def _run(c):
    """make -> ops call on the contiguous middles of the guarded device buffers -> verify.  The wrappers take such
    slices as they are (they check contiguity and copy nothing), so the kernel reads and writes the guarded buffers."""
    from visual_onoma_to_wave_amd import _lib
    m = RC.make(c)
    ref, bar = RC.reference(c, m)
    dev = torch.device("cuda:0")
    B = c["B"]
    x_buf, y_buf = m["x_buf"].to(dev), m["y_buf"].to(dev)
    acc_buf = m["acc_buf"].to(dev) if m["acc_buf"] is not None else None
    d = {k: [t.to(dev) for t in m[k]] for k in ("p1", "p2", "b1", "b2")}
    d["x"], d["y"] = x_buf[1:B + 1], y_buf[1:B + 1]
    d["acc"] = d["y"] if c["acc"] == "mrf" else (acc_buf[1:B + 1] if acc_buf is not None else None)
    assert d["x"].is_contiguous() and d["y"].is_contiguous() and d["x"].data_ptr() == x_buf.data_ptr() + x_buf[0].numel() * 2
    knob = c["knob"]
    if knob:
        _lib.lib().vo_tune(knob[0].encode(), knob[1])
    try:
        out = _call(c, d)
        torch.cuda.synchronize()
    finally:
        if knob:
            _lib.lib().vo_tune(knob[0].encode(), 0)
    assert out is d["y"], f"{c['name']}: the entry did not run the call"
    m["x_buf"].copy_(x_buf.cpu())
    m["y_buf"].copy_(y_buf.cpu())
    if acc_buf is not None:
        m["acc_buf"].copy_(acc_buf.cpu())
    return RC.verify(c, m, ref, bar)


# the lengths are functions of the built kernels' tiles: the ids name them, the test asks the library
@pytest.mark.parametrize("route,dils,length,acc", RC.matrix_ids(),
                         ids=[f"{r}-d{'_'.join(map(str, d))}-{lid}-{a}" for r, d, lid, a in RC.matrix_ids()])
def test_resblock_edge(route, dils, length, acc):
    entry, C, K, _, knob, _ = RC.routes()[route]
    bt = _tile_rows(route, entry, C, K, dils, knob)
    assert bt > 0
    _run(RC.matrix_case(route, dils, length, acc, bt))


@pytest.mark.parametrize("K", [7, 11])
def test_resblockk_epilogue_add_is_not_handled(K):
    """vo_resblockk has no epilogue-add accumulator mode: with an out_scale whose inverse is no bf16 value (0.3) it
    returns VO_NOT_HANDLED -- ops.resblock_k returns None -- and writes nothing, guard utterances and view alike."""
    from visual_onoma_to_wave_amd import ops
    c = RC.case("blockk", 3, RC.halo(dict(K=K, dils=(1, 3, 5))) + 1, 32, K, (1, 3, 5), acc="add")
    m = RC.make(c)
    dev = torch.device("cuda:0")
    x_buf, y_buf, acc_buf = m["x_buf"].to(dev), m["y_buf"].to(dev), m["acc_buf"].to(dev)
    d = {k: [t.to(dev) for t in m[k]] for k in ("p1", "p2", "b1", "b2")}
    out = ops.resblock_k(x_buf[1:4], d["p1"], d["b1"], d["p2"], d["b2"], K, c["dils"], c["slope"], out=y_buf[1:4],
                         out_scale=c["out_scale"], acc=acc_buf[1:4])
    torch.cuda.synchronize()
    assert out is None
    assert bool((y_buf.cpu().view(torch.int16) == RC.BF16_GUARD).all())
    assert torch.equal(acc_buf.cpu().view(torch.int16), m["acc_orig"].view(torch.int16))
