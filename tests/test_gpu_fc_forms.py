"""Every case of tests/_fc_cases.py on the device.  Needs an MI355X.

What the shape lists of tests/test_gpu_heads.py cannot see (tests/test_fc_plan.py proves on the host that these cases
do): every kernel form and instantiation of csrc/gemm.hip, the selector's fallbacks (float4 loads from 4-byte aligned
addresses), ragged last tiles in M and N, the weight padding up to Npad, device row counts of 0, inside a tile, M and
beyond M on every kernel.  Each case first asserts that the built layer selects what the host plan says
(FullyConnected.form == ops.fc_plan_host, nothing launched), then runs the call as the API is used.

'int' data is compared bit for bit with the float64 product rounded once: every k used exactly once.  'normal' data
is held to test_gpu_heads.py's bars.  Every case checks on the raw bits that nothing outside [:rows, :N] of y changed,
with x's padding and surplus rows NaN.  Layers are shared by the cases of one (K, N, dtype, relu, data) and called back
to back."""
import os

import numpy as np
import pytest

import _fc_cases as fcc
from dodt_amd import _lib, device, ops
from oracle import tfops

pytestmark = pytest.mark.gpu

# the library reads the switch once per process (tests/test_gpu_variants.py runs the bf16-row cases under 64)
BF16_BK = 64 if os.environ.get('DODT_FC_BF16_DMA_BK') == '64' else 32


@pytest.fixture(scope='module')
def ctx():
    return device.default_context()


@pytest.fixture(scope='module')
def layers(ctx):
    made = {}

    def get(c):
        key = fcc.layer_key(c)
        if key not in made:
            w, b = fcc.layer_params(key)
            made[key] = ops.FullyConnected(ctx, w, b, c.relu, dtype=c.dtype)
        return made[key]

    yield get
    for fc in made.values():
        fc.close()


def _at(ctx, host, off):
    """`host` on the device, `off` bytes into an allocation of its own: (the allocation, the view)."""
    raw = ctx.empty((host.nbytes + 16,), np.uint8)
    assert raw.ptr % 16 == 0 and 0 <= off < 16
    view = raw.offset(off, host.shape, host.dtype)
    view.upload(host)
    return raw, view


def _bf16_rows(ctx, fc, c, x):
    """The rows the bf16 heads feed a layer: ops.rows_to_bf16 of the float32 rows, dense; as uint16 on the host."""
    elems = fc.bf16_row_elems()
    assert elems == (-(-c.K // 64) * 64 if fcc.group(fcc.host_plan(c)['name']) == 'bf16_rows_dma' else c.K)
    d_rows = ctx.array(np.full((c.M, elems), fcc.NAN16, np.uint16))
    ops.rows_to_bf16(ctx, ctx.array(x), None, c.M, None, c.K, c.K, d_rows, elems)
    rows = d_rows.download()
    assert np.array_equal(ops.bf16_to_float(rows[:, :c.K]), tfops.round_bf16(x)) and not rows[:, c.K:].any()
    return rows


def _run(ctx, fc, c):
    """The case's call on layer fc: asserts the form, returns the raw bits of the output arrays."""
    x, x2 = fcc.case_inputs(c)
    bf16_rows = c.entry in ('bf16', 'split_bf16')
    split = c.entry in ('split', 'split_bf16')
    keep = []
    if bf16_rows:
        assert not c.fuse
        ximg = fcc.x_image(c, _bf16_rows(ctx, fc, c, x), fc.bf16_row_elems())
    else:
        ximg = fcc.x_image(c, x)
    raw, d_x = _at(ctx, ximg, c.x_off)
    keep.append(raw)
    d_x2 = None
    if c.fuse:
        raw, d_x2 = _at(ctx, fcc.x_image(c, x2), c.x2_off)
        keep.append(raw)
    d_ys = []
    for alloc, ld, _ in fcc.y_shapes(c):
        img = np.full((alloc, ld), fcc.y_sentinel(c), np.uint16 if c.y_bf16 else np.uint32)
        raw, d_y = _at(ctx, img, 0 if split else c.y_off)
        keep.append(raw)
        d_ys.append(d_y)
    d_m = None if c.d_m is None else ctx.array(np.array([c.d_m], np.int32))

    want = fcc.host_plan(c, BF16_BK)
    assert want['name'] == fcc.expected_form(c, BF16_BK)
    got = fc.form(d_x, c.M, None if split else d_ys[0], ldx=c.ldx, ldy=c.ldy, d_x2=d_x2, x_bf16=bf16_rows,
                  y_bf16=c.y_bf16)
    assert got == want, 'the layer selects something else than dodt_fc_plan_host'

    if c.entry == 'forward':
        fc.forward(d_x, c.M, d_ys[0], ldx=c.ldx, ldy=c.ldy, d_x2=d_x2, d_m=d_m)
    elif c.entry == 'split':
        assert fc.can_split(c.ldx)
        fc.forward_split(d_x, c.M, d_ys, c.widths, ldx=c.ldx, d_m=d_m)
    elif c.entry == 'bf16':
        fc.forward_bf16(d_x, c.M, d_ys[0], ldx=c.ldx, ldy=c.ldy, d_m=d_m, y_bf16=c.y_bf16)
    else:
        fc.forward_split_bf16(d_x, c.M, d_ys, c.widths, ldx=c.ldx, d_m=d_m)
    return [d_y.download() for d_y in d_ys]


@pytest.mark.parametrize('c', fcc.CASES, ids=[c.name for c in fcc.CASES])
def test_fc_form_case(ctx, layers, c):
    images = _run(ctx, layers(c), c)
    want = fcc.reference(c)
    n = fcc.rows(c)
    if n:
        got = fcc.y_values(c, np.ascontiguousarray(images[0][:n, :fcc.y_shapes(c)[0][2]]))
        ref = fcc.output_value(c, want[:n, :got.shape[1]])
        print('%s: rows %d, max |got - want| %g at scale %g' % (c.name, n, np.abs(got - ref).max(), np.abs(ref).max()))
    assert fcc.check_outputs(c, images, want) == []


@pytest.mark.parametrize('c', fcc.REFUSED, ids=[c.name for c in fcc.REFUSED])
def test_fc_refused_bf16_rows(ctx, c):
    """bf16 rows no kernel of the layer reads: the host plan says kNone, the built layer says the same, and the entry
    raises before any launch (y keeps its bits)."""
    assert fcc.host_plan(c, BF16_BK)['name'] == 'kNone'
    w, b = fcc.layer_params(fcc.layer_key(c))
    fc = ops.FullyConnected(ctx, w, b, c.relu, dtype=c.dtype)
    try:
        assert fc.bf16_row_elems() == (c.K if c.N <= 32 else 0)
        d_x = ctx.array(np.zeros((c.M + 1, c.ldx), np.uint16))
        alloc, ld, _ = fcc.y_shapes(c)[0]
        d_y = ctx.array(np.full((alloc, ld), fcc.y_sentinel(c), np.uint16 if c.y_bf16 else np.uint32))
        assert fc.form(d_x, c.M, d_y, ldx=c.ldx, ldy=c.ldy, x_bf16=True, y_bf16=c.y_bf16) == fcc.host_plan(c, BF16_BK)
        with pytest.raises(_lib.DodtError, match='dodt_fc_forward_bf16'):
            fc.forward_bf16(d_x, c.M, d_y, ldx=c.ldx, ldy=c.ldy, y_bf16=c.y_bf16)
        ctx.sync()
        assert (d_y.download() == fcc.y_sentinel(c)).all()
    finally:
        fc.close()
