"""Row-operand epilogues of the d8 GEMM (gated residual = epilogue 2, GELU adjoint = epilogue 3) after the round-7 restructuring: bias and gate
values are gathered before a tile's first store and handed out by ds_bpermute, the residual rows roll one 64-column group ahead.  Only data
movement changed, so every output must stay bit-identical to gemm_t8_kernel's on the same operands, and inside the project's per-op bound
against fp32: |err| <= 1.6e-2 |ref| + 1e-2 max|ref|.

The t8 kernel needs K % 128 == 0 and the d8 kernel K % 192 == 0: at K = 192 and K = 576 there is no t8 launch to compare with.  Those cases
are checked against fp32 and for bit-identity between the d8 tile widths (the accumulation order of an output element does not depend on the
width); every case is repeated at K = 384, where both kernels run, with torch.equal against t8.  192-row tiles are refused where they would
leave the packed row slots (M = 400: 3 x 192 > 512), so the 192-row bodies run at M = 700 (3 x 192 + 124 rows: a ragged last tile)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
SEQ, N_TEXT, PER_GROUP = 111, 7, 13          # 16-row blocks inside one token group, across one boundary and across two (13-row groups)
N_GROUPS = 1 + -(-(SEQ - N_TEXT) // PER_GROUP)


def _dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def _pinned(ring, bm, bn, fn):
    from orv_amd._lib import lib
    lib().orv_gemm_force_tile(ring, bm, bn)
    try:
        return fn()
    finally:
        lib().orv_gemm_force_tile(0, 0, 0)


def _same(a, b, what):
    assert torch.equal(a.view(torch.int16), b.view(torch.int16)), (what, (a.float() - b.float()).abs().max().item())


def _close(got, ref, what):
    got, ref = got.float(), ref.float()
    err, bound = (got - ref).abs(), 1.6e-2 * ref.abs() + 1e-2 * ref.abs().max()
    assert torch.isfinite(got).all() and (err <= bound).all(), (what, err.max().item(), ref.abs().max().item())


def _group_of_rows(rows):
    s = rows % SEQ
    return rows // SEQ, torch.where(s < N_TEXT, torch.zeros_like(s), 1 + (s - N_TEXT).clamp(min=0) // PER_GROUP)


class _Case:
    """One set of operands; `run` launches epilogue 2 / 3 on the pinned kernel, `ref` is the fp32 restatement (computed once)."""

    def __init__(self, M, N, K, seed, bias=True, gate=True, inplace=False, cmap=False, r_mod=0, epi=2):
        from orv_amd import ops
        dev = _dev()
        g = torch.Generator(device=dev).manual_seed(seed)
        self.M, self.N, self.K, self.epi, self.inplace, self.r_mod = M, N, K, epi, inplace, r_mod
        self.A = torch.randn(M, K, device=dev, generator=g).to(BF)
        self.W = (torch.randn(N, K, device=dev, generator=g) / K ** 0.5).to(BF)
        self.bias = torch.randn(N, device=dev, generator=g).to(BF) if bias else None
        self.Ap = ops.pack_rows16(self.A, M, K)
        self.cmap = ops.RowMap(SEQ - N_TEXT, SEQ, N_TEXT) if cmap else None
        rows = torch.arange(M, device=dev)
        self.orow = rows // (SEQ - N_TEXT) * SEQ + N_TEXT + rows % (SEQ - N_TEXT) if cmap else rows
        self.rows_out = int(self.orow.max().item()) + 1
        batches = -(-self.rows_out // SEQ)
        self.gate = torch.randn(batches, N_GROUPS, N, device=dev, generator=g) if gate else None
        self.R = torch.randn(r_mod if r_mod else self.rows_out, N, device=dev, generator=g).to(BF)
        acc = self.A.float() @ self.W.float().t() + (self.bias.float() if bias else 0.)
        self.ref_y = acc
        res = self.R.float()[rows % r_mod] if r_mod else self.R.float()[self.orow]
        if epi == 2:
            if gate:
                b, grp = _group_of_rows(self.orow)
                acc = self.gate[b, grp] * acc
            self.ref_c = res + acc
        else:
            x = res.clone().requires_grad_(True)
            torch.nn.functional.gelu(x, approximate="tanh").sum().backward()
            self.ref_c = acc * x.grad

    def run(self, ring, bm, bn):
        from orv_amd import ops
        dev = self.A.device
        packed = ring == 5
        C = self.R.clone() if self.inplace else torch.full((self.rows_out, self.N), float("nan"), dtype=BF, device=dev)
        Y = torch.full((self.rows_out, self.N), float("nan"), dtype=BF, device=dev)
        kw = dict(R=C if self.inplace else self.R, ldr=self.N, r_mod=self.r_mod, a_packed=packed, Y=Y, cmap=self.cmap)
        if self.gate is not None:
            kw.update(gate=self.gate, gate_b=N_GROUPS * self.N, gate_g=self.N, grp=ops.Groups(SEQ, N_TEXT, PER_GROUP))
        _pinned(ring, bm, bn, lambda: ops.gemm(self.Ap if packed else self.A, self.W, self.bias, C, self.M, self.N, self.K,
                                               epilogue=self.epi, **kw))
        return C[self.orow], Y[self.orow]

    def check(self, widths, bm=256, what=""):
        outs = [self.run(5, bm, bn) for bn in widths]
        for bn, (c, y) in zip(widths, outs):
            _close(c, self.ref_c, (what, bn, "C")), _close(y, self.ref_y, (what, bn, "Y"))
            _same(c, outs[0][0], (what, bn, "C across widths")), _same(y, outs[0][1], (what, bn, "Y across widths"))
        if self.K % 128 == 0:
            for bn, (c, y) in zip(widths, outs):
                if bn < 192:             # no 128-column t8 tile: that width is compared with the 192-column d8 kernel above
                    assert 192 in widths
                    continue
                c0, y0 = self.run(3, 256, bn)
                _same(c, c0, (what, bn, "C vs t8")), _same(y, y0, (what, bn, "Y vs t8"))
        return outs[0]


@pytest.mark.parametrize("K", [192, 384, 576])
def test_gated_residual_small_ragged(K):
    """M = 333 (two row tiles, invalid rows), N = 384: bias / gate on and off, residual in place and apart, Y on."""
    for i, (bias, gate, inplace) in enumerate([(True, True, False), (True, True, True), (False, True, False), (True, False, True),
                                               (False, False, False)]):
        _Case(333, 384, K, 700 + i, bias=bias, gate=gate, inplace=inplace).check((128, 192), what=(K, bias, gate, inplace))


@pytest.mark.parametrize("K", [192, 384])
def test_gated_residual_row_maps(K):
    """A table residual (r_mod) and an output row map (video rows scattered into the joint buffer, gate rows found through the map)."""
    _Case(333, 384, K, 720, gate=False, r_mod=97).check((128, 192), what=(K, "r_mod"))
    _Case(312, 384, K, 721, cmap=True).check((128, 192), what=(K, "row map"))
    _Case(312, 384, K, 722, cmap=True, inplace=True).check((128, 192), what=(K, "row map, in place"))


@pytest.mark.parametrize("K", [192, 384])
def test_gated_residual_more_tiles_than_cus(K):
    """Workgroups that run an interior epilogue and then another tile: the next tile's loads are in flight across the epilogue."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    _Case(256 * (cus // 10 + 2), 1920, K, 730).check((192, 128), what=(K, "tiles > CUs"))


def test_gated_residual_256_column_tiles():
    _Case(333, 512, 384, 740).check((256,), what="bn 256")
    _Case(333, 512, 384, 741, inplace=True, bias=False).check((256,), what="bn 256, in place")
    # more tiles than CUs: the 256-column kernel reads the next tile's first W fragments again behind its epilogue
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    _Case(256 * (cus // 10 + 2), 2560, 384, 742).check((256,), what="bn 256, tiles > CUs")
    _Case(256 * (cus // 10 + 2), 2560, 384, 743, gate=False, epi=3).check((256,), what="bn 256, tiles > CUs, epi 3")


@pytest.mark.parametrize("K", [192, 384, 576])
def test_gelu_adjoint(K):
    """Epilogue 3 (192- and 256-column tiles exist)."""
    _Case(333, 384, K, 750, gate=False, epi=3).check((192,), what=(K, "epi 3"))
    _Case(333, 384, K, 751, gate=False, bias=False, epi=3).check((192,), what=(K, "epi 3, no bias"))
    _Case(333, 512, K, 752, gate=False, epi=3).check((256,), what=(K, "epi 3, bn 256"))


@pytest.mark.parametrize("bn", [128, 192])
def test_gated_residual_192_row_bodies(bn):
    """gemm_d8r192_kernel<bn, 2>: both wave roles (two row blocks / one) against the 256-row kernel and t8."""
    case = _Case(700, 384, 384, 760 + bn)
    c0, y0 = case.check((192, bn), what=(bn, "256 rows"))
    c1, y1 = case.run(5, 192, bn)
    _same(c1, c0, (bn, "192-row C")), _same(y1, y0, (bn, "192-row Y"))
    case = _Case(624, 384, 192, 770 + bn, cmap=True, inplace=True)
    c0, y0 = case.check((192, bn), what=(bn, "256 rows, row map"))
    c1, y1 = case.run(5, 192, bn)
    _same(c1, c0, (bn, "192-row C, row map")), _same(y1, y0, (bn, "192-row Y, row map"))


def test_gated_residual_repeats():
    case = _Case(333, 384, 576, 780)
    first = case.run(5, 256, 192)
    for _ in range(2):
        again = case.run(5, 256, 192)
        _same(again[0], first[0], "C repeat"), _same(again[1], first[1], "Y repeat")
