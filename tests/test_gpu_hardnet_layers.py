"""Every stock-HardNet train kernel alone against fp64 (hn_hardnet_train_layer_op), one layer and one form at a time:
the cases, references and bars are tests/hardnet_layer_ref.py's (tests/test_hardnet_layer_ref.py shows on the CPU that
no structural error fits under them).  Forms are chosen in-process through the entry's HN_TRAIN_F32 bits argument,
row segments and column chunks through its overrides.  Every output sits between canaries and starts as NaN bytes;
the scratch sits between canaries and is pre-filled once with 0x00 and once with 0xFF bytes, which must not change a
bit of the result.  The last test chains the entry's operations in the step's order and must reproduce
hn_hardnet_train_forward / _backward bit for bit: the entry is the product's own code."""
import pytest
import torch

import hardnet_layer_ref as R
from hardnetnas_amd import _native as N

pytestmark = pytest.mark.gpu


def guarded(nbytes, dev, fill):
    """tests/test_gpu_det_train.py's helper: a uint8 tensor of ``nbytes`` (rounded up to 16) inside a larger allocation
    with 256 canary bytes either side."""
    n = (nbytes + 15) // 16 * 16
    whole = torch.full((n + 512,), 0xA5, dtype=torch.uint8, device=dev)
    whole[256:256 + n] = fill
    return whole, whole[256:256 + n]


def intact(whole):
    return bool((whole[:256] == 0xA5).all()) and bool((whole[-256:] == 0xA5).all())


# HN_TRAIN_F32 bits (csrc/hn_internal.h): 1 f32 forwards (else bf16x3), 2 stride-1 dgrads f32 (else bf16x3),
# 4 stride-1 wgrads generic, 8 stride-1 forwards generic, 16 stride-1 dgrads not k_fwd3, 32 stride-2 generic,
# 64 conv0 generic, 128 swaps one-ring and shared-ring.  NS: the row-segment counts passed; a count above what the
# geometry allows is clamped by the launcher (conv5 / conv4: 4 -> 2), so it must equal the clamped form bit for bit.
NS = (1, 2, 4)
FORMS = {
    ("conv_fwd", 0): [("k_fwd0", 17, (0,)), ("gemm", 17 | 64, (0,))],
    ("conv_fwd", 1): [("k_fwd3", 1, NS), ("bf16x3", 0, (0,)), ("gemm", 1 | 8, (0,))],
    ("conv_fwd", 2): [("k_fwd2 one-ring", 1, NS), ("k_fwd2 shared", 1 | 128, NS), ("bf16x3", 0, (0,)),
                      ("gemm", 1 | 32, (0,))],
    ("conv_fwd", 3): [("k_fwd3s shared", 1, NS), ("k_fwd3 one-ring", 1 | 128, NS), ("bf16x3", 0, (0,)),
                      ("gemm", 1 | 8, (0,))],
    ("conv_fwd", 4): [("k_fwd2 shared", 1, NS), ("k_fwd2 one-ring", 1 | 128, NS), ("bf16x3", 0, (0,)),
                      ("gemm", 1 | 32, (0,))],
    ("conv_fwd", 5): [("k_fwd3s shared", 1, NS), ("k_fwd3 one-ring", 1 | 128, NS), ("bf16x3", 0, (0,)),
                      ("gemm", 1 | 8, (0,))],
    ("conv_fwd", 6): [("gemm", 17, (0,))],
    ("conv_wgrad", 0): [("k_wgrad0", 17, (0,)), ("gemm", 17 | 64, (0,))],
    ("conv_wgrad", 1): [("k_wgrad3", 17, NS), ("gemm", 17 | 4, (0,))],
    ("conv_wgrad", 2): [("k_wgrad2", 17, NS), ("gemm", 17 | 32, (0,))],
    ("conv_wgrad", 3): [("k_wgrad3", 17, NS), ("gemm", 17 | 4, (0,))],
    ("conv_wgrad", 4): [("k_wgrad2", 17, NS), ("gemm", 17 | 32, (0,))],
    ("conv_wgrad", 5): [("k_wgrad3", 17, NS), ("gemm", 17 | 4, (0,))],
    ("conv_wgrad", 6): [("gemm", 17, (0,))],
    ("conv_dgrad", 0): [("gemm", 17, (0,))],
    ("conv_dgrad", 1): [("k_fwd3", 1, NS), ("bf16x3", 17, (0,)), ("gemm", 19, (0,))],
    ("conv_dgrad", 2): [("k_dgrad2", 17, NS), ("col2im", 17 | 32, (0,))],
    ("conv_dgrad", 3): [("k_fwd3s shared", 1, NS), ("k_fwd3 one-ring", 1 | 128, NS), ("bf16x3", 17, (0,)),
                        ("gemm", 19, (0,))],
    ("conv_dgrad", 4): [("k_dgrad2 shared", 17, NS), ("k_dgrad2 one-ring", 17 | 128, NS), ("col2im", 17 | 32, (0,))],
    ("conv_dgrad", 5): [("k_fwd3s shared", 1, NS), ("k_fwd3 one-ring", 1 | 128, NS), ("bf16x3", 17, (0,)),
                        ("gemm", 19, (0,))],
    ("conv_dgrad", 6): [("col6", 17, (0,))],
}
NAN_BYTE = 0xFF


class Hook:
    """hn_hardnet_train_layer_op with a guarded scratch (filled per call) and guarded outputs."""

    def __init__(self, dev, batch, bits=-1, row_segments=0):
        self.dev, self.batch, self.bits, self.ns = dev, batch, bits, row_segments
        self.need = N.train_layer_op_workspace_bytes(batch, bits, row_segments)

    def out(self, shape, init=None):
        """(whole, view): a float32 tensor between canaries, NaN bytes or ``init``."""
        n = 1
        for s in shape:
            n *= s
        whole, buf = guarded(4 * n, self.dev, NAN_BYTE)
        view = buf[:4 * n].view(torch.float32).view(shape)
        if init is not None:
            view.copy_(init)
        return whole, view

    def run(self, op, layer, fill, x=None, w=None, y=None, aux=(None, None, None), **kw):
        whole, scratch = guarded(self.need, self.dev, fill)
        N.train_layer_op(op, layer, self.batch, x, w, y, aux, bits=self.bits, row_segments=self.ns, scratch=scratch,
                         **kw)
        torch.cuda.synchronize(self.dev)
        assert intact(whole), f"{op} layer {layer}: wrote outside its scratch"


def dev_cnhw(t, dev):
    return R.to_cnhw(t).to(dev)


def run_conv(case, dev, bits, ns, chunk=0):
    """The convolution case under one form: the result as NCHW on the CPU, the same bits for both scratch fills."""
    op, l, b = case
    kind = op.split("+")[0]
    x = R.conv_case(case)["x"]
    cin, cout, h, k, s, p = R.LAYERS[l]
    ho = R.hout(l)
    z, w, dy = dev_cnhw(x["z"], dev), x["w"].to(dev), dev_cnhw(x["dy"], dev)
    kw = {"dgrad_chunk": chunk}
    if x["mask"] is not None:
        kw.update(dropout_p=R.DROP_P, seed=R.DROP_SEED)
    hook = Hook(dev, b, bits, ns)
    results = []
    for fill in (0x00, 0xFF):
        if kind == "conv_fwd":
            whole, y = hook.out((cout, b, ho, ho))
            hook.run(kind, l, fill, z, w, y, **kw)
        elif kind == "conv_wgrad":
            whole, y = hook.out((cout, cin, k, k))
            hook.run(kind, l, fill, z, dy, y, **kw)
        else:
            whole, y = hook.out((cin, b, h, h))
            hook.run(kind, l, fill, dy, w, y, **kw)
        assert intact(whole), f"{R.case_id(case)}: wrote outside its output"
        results.append(y.clone())
    assert torch.equal(results[0].view(torch.int32), results[1].view(torch.int32)), \
        f"{R.case_id(case)} bits {bits} NS {ns}: the result depends on what the scratch held"
    got = results[0].cpu()
    return got if kind == "conv_wgrad" else R.from_cnhw(got)


@pytest.mark.parametrize("case", R.CONV_CASES, ids=R.case_id)
def test_convolution_forms(case, cuda_device):
    op, l, b = case
    c = R.conv_case(case)
    failures = []
    for form, bits, ns_list in FORMS[(op, l)]:
        bar = c["bar_bf16x3"] if form == "bf16x3" else c["bar"]
        got = {ns: run_conv(case, cuda_device, bits, ns) for ns in ns_list}
        for ns, g in got.items():
            if not R.check(f"{R.case_id(case)} {form} NS={ns}", g, c["ref64"], bar, c["e32"]):
                failures.append((form, ns))
        first = got[ns_list[0]]
        for ns in ns_list[1:]:
            if op == "conv_wgrad":
                # the row segments regroup the products into other split-K slices (fp32 within a slice, fp64 across:
                # k_splitk_sum), so the counts agree at the bar, not bit for bit
                d = R.metrics(got[ns], first)
                print(f"[hardnet-layer] {R.case_id(case)} {form} NS={ns} vs NS={ns_list[0]}: L2 {d[0]:.3e} max {d[1]:.3e}")
                assert d[0] <= bar[0] and d[1] <= bar[1], (form, ns)
            else:
                assert torch.equal(got[ns].view(torch.int32), first.view(torch.int32)), \
                    f"{form}: NS={ns} differs from NS={ns_list[0]} (every output keeps its K order)"
    assert not failures, failures


@pytest.mark.parametrize("layer,bits", [(2, 17 | 32), (4, 17 | 32), (6, 17)])
def test_column_gemm_data_gradient_in_chunks(layer, bits, cuda_device):
    """dgrad_chunk = 2 at B = 5: three chunks, the last one ragged; the same bits as one chunk."""
    case = ("conv_dgrad", layer, 5)
    c = R.conv_case(case)
    whole = run_conv(case, cuda_device, bits, 0)
    chunks = run_conv(case, cuda_device, bits, 0, chunk=2)
    assert R.check(f"{R.case_id(case)} column GEMM, chunks of 2", chunks, c["ref64"], c["bar"], c["e32"])
    assert R.check(f"{R.case_id(case)} column GEMM, one chunk", whole, c["ref64"], c["bar"], c["e32"])
    assert torch.equal(chunks.view(torch.int32), whole.view(torch.int32))


@pytest.mark.parametrize("case", [c for c in R.DROPOUT_CASES if c[0].startswith("conv")], ids=R.case_id)
def test_layer6_with_dropout(case, cuda_device):
    """conv6's loader applies the counter-hash mask to relu(z5); the fp64 reference applies its restatement."""
    c = R.conv_case(case)
    assert 0.2 < float((c["x"]["mask"] == 0).float().mean()) < 0.4
    got = run_conv(case, cuda_device, 17, 0)
    assert R.check(f"{R.case_id(case)} gemm", got, c["ref64"], c["bar"], c["e32"])


@pytest.mark.parametrize("case", R.BN_CASES + [c for c in R.DROPOUT_CASES if c[0].startswith("bn")], ids=R.case_id)
def test_batchnorm(case, cuda_device):
    op, l, b = case
    dev = cuda_device
    c = R.bn_case(case)
    x = c["x"]
    hook = Hook(dev, b)
    ns = R.bn_slices(R.LAYERS[l][1], b * R.hout(l) ** 2)[0]
    print(f"[hardnet-layer] {R.case_id(case)}: {ns} statistics slice(s)")
    results = []
    for fill in (0x00, 0xFF):
        if op == "bn_fwd":
            wy, y = hook.out(R.to_cnhw(x["y"]).shape, R.to_cnhw(x["y"]))
            wr, rstd = hook.out(x["rmean"].shape)
            wm, rmean = hook.out(x["rmean"].shape, x["rmean"])
            wv, rvar = hook.out(x["rvar"].shape, x["rvar"])
            hook.run("bn_fwd", l, fill, None, None, y, (rstd, rmean, rvar), momentum=R.MOMENTUM)
            assert all(intact(w) for w in (wy, wr, wm, wv))
            results.append([R.from_cnhw(y.cpu()), rstd.cpu(), rmean.cpu(), rvar.cpu()])
        else:
            wy, g = hook.out(R.to_cnhw(x["da"]).shape, R.to_cnhw(x["da"]))
            kw = {"dropout_p": R.DROP_P, "seed": R.DROP_SEED} if x["mask"] is not None else {}
            hook.run("bn_bwd", l, fill, dev_cnhw(x["z"], dev), x["rstd"].to(dev), g, **kw)
            assert intact(wy)
            results.append([R.from_cnhw(g.cpu())])
    for a, bb in zip(*results):
        assert torch.equal(a.view(torch.int32), bb.view(torch.int32))
    got = results[0]
    if op == "bn_fwd":
        ok = R.check(f"{R.case_id(case)} z", got[0], c["ref64"][0], c["bar"][0], c["e32"][0])
        ok &= R.check(f"{R.case_id(case)} rstd", got[1], c["ref64"][1], c["bar"][1], c["e32"][1])
        ok &= R.check_running(f"{R.case_id(case)} running_mean", got[2], c["ref64"][2])
        ok &= R.check_running(f"{R.case_id(case)} running_var", got[3], c["ref64"][3])
        # without running statistics: the same z and rstd
        wy, y = hook.out(R.to_cnhw(x["y"]).shape, R.to_cnhw(x["y"]))
        wr, rstd = hook.out(x["rmean"].shape)
        hook.run("bn_fwd", l, 0xFF, None, None, y, (rstd, None, None), momentum=R.MOMENTUM)
        assert intact(wy) and intact(wr)
        assert torch.equal(R.from_cnhw(y.cpu()), got[0]) and torch.equal(rstd.cpu(), got[1])
    else:
        ok = R.check(f"{R.case_id(case)} relu={l < 6}", got[0], c["ref64"], c["bar"], c["e32"])
    assert ok


@pytest.mark.parametrize("case", R.PATCH_CASES, ids=R.case_id)
def test_per_patch_kernels(case, cuda_device):
    op, _, b = case
    dev = cuda_device
    c = R.patch_case(case)
    x = {k: v.to(dev) for k, v in c["x"].items()}
    hook = Hook(dev, b)
    results = []
    for fill in (0x00, 0xFF):
        if op == "input_norm":
            w0, xn = hook.out((b, 1024))
            w1, inv = hook.out((b,))
            hook.run(op, 0, fill, x["x"], None, xn, (inv, None, None))
            outs, wholes = [xn.cpu(), inv.cpu()], (w0, w1)
        elif op == "input_norm_bwd":
            w0, g = hook.out((b, 1024), x["g"])
            w1, din = hook.out((b, 1024))
            hook.run(op, 0, fill, x["inv_sd"], None, g, (din, None, None))
            assert torch.equal(g, din)  # the scaled gradient and its copy
            outs, wholes = [din.cpu()], (w0, w1)
        elif op == "l2_fwd":
            w0, y = hook.out((b, 128))
            hook.run(op, 0, fill, x["z"].t().contiguous(), None, y)
            outs, wholes = [y.cpu()], (w0,)
        else:
            w0, dz = hook.out((128, b))
            hook.run(op, 0, fill, x["z"].t().contiguous(), x["dout"], dz)
            outs, wholes = [dz.cpu().t().contiguous()], (w0,)
        assert all(intact(w) for w in wholes)
        results.append(outs)
    for a, bb in zip(*results):
        assert torch.equal(a.view(torch.int32), bb.view(torch.int32))
    ok = True
    for i, got in enumerate(results[0]):
        ok &= R.check(f"{R.case_id(case)} output {i}", got, c["ref64"][i], c["bar"][i], c["e32"][i])
    assert ok


def test_chained_operations_are_the_product_step(cuda_device):
    """B = 37, the process's own HN_TRAIN_F32 bits, no overrides, dropout on: the entry's operations chained in the
    step's order give the descriptors, the seven weight gradients, the input gradient and the running statistics of
    hn_hardnet_train_forward / _backward bit for bit."""
    dev, b = cuda_device, 37
    case = ("chain", 0, b)
    inp = torch.from_numpy(R.synth.synth_patches(b, seed=37)).reshape(b, 1024).to(dev)
    ws = [(R.normal(case, f"w{l}", (co, ci, k, k)) / float(ci * k * k) ** 0.5).to(dev)
          for l, (ci, co, h, k, s, p) in enumerate(R.LAYERS)]
    dout = R.normal(case, "dout", (b, 128)).to(dev)
    stats0 = [(0.1 * R.normal(case, f"rm{l}", (L[1],)), 1.0 + 0.2 * R.normal(case, f"rv{l}", (L[1],)).abs())
              for l, L in enumerate(R.LAYERS)]
    p, seed = R.DROP_P, R.DROP_SEED

    # the product
    rm_p, rv_p = [m.clone().to(dev) for m, _ in stats0], [v.clone().to(dev) for _, v in stats0]
    n_sv, n_sc = N.train_workspace_bytes(b)
    saved = torch.empty(n_sv, device=dev, dtype=torch.uint8)
    scratch = torch.empty(n_sc, device=dev, dtype=torch.uint8)
    out_p = torch.empty((b, 128), device=dev)
    N._call(dev, "hn_hardnet_train_forward", inp, b, N._ptr_array(ws), N._ptr_array(rm_p), N._ptr_array(rv_p),
            R.MOMENTUM, p, seed, out_p, *N._buf(saved), *N._buf(scratch))
    dws_p = [torch.empty_like(w) for w in ws]
    din_p = torch.empty((b, 1024), device=dev)
    N._call(dev, "hn_hardnet_train_backward", dout, b, N._ptr_array(ws), N._ptr_array(dws_p), din_p, p, seed,
            *N._buf(saved), *N._buf(scratch))

    # the same step, one operation per call
    sc = torch.empty(N.train_layer_op_workspace_bytes(b), device=dev, dtype=torch.uint8)
    op = lambda name, l, x, w, y, aux=(None, None, None): N.train_layer_op(  # noqa: E731
        name, l, b, x, w, y, aux, momentum=R.MOMENTUM, dropout_p=p, seed=seed, scratch=sc)
    new = lambda *shape: torch.full(shape, float("nan"), device=dev)  # noqa: E731
    rm_h, rv_h = [m.clone().to(dev) for m, _ in stats0], [v.clone().to(dev) for _, v in stats0]
    xn, inv_sd = new(b, 1024), new(b)
    op("input_norm", 0, inp, None, xn, (inv_sd, None, None))
    zs, rstds = [], []
    for l, (ci, co, h, k, s, pad) in enumerate(R.LAYERS):
        z = op("conv_fwd", l, xn if l == 0 else zs[-1], ws[l], new(co, b, R.hout(l), R.hout(l)))
        rstds.append(new(co))
        op("bn_fwd", l, None, None, z, (rstds[-1], rm_h[l], rv_h[l]))
        zs.append(z)
    out_h = op("l2_fwd", 0, zs[6], None, new(b, 128))
    g = op("l2_bwd", 0, zs[6], dout, new(128, b))
    dws_h = [None] * 7
    for l in range(6, -1, -1):
        ci, co, h, k, s, pad = R.LAYERS[l]
        op("bn_bwd", l, zs[l], rstds[l], g)
        a = xn if l == 0 else zs[l - 1]
        dws_h[l] = op("conv_wgrad", l, a, g, new(co, ci, k, k))
        g = op("conv_dgrad", l, g, ws[l], new(ci, b, h, h))
    din_h = new(b, 1024)
    op("input_norm_bwd", 0, inv_sd, None, g, (din_h, None, None))
    torch.cuda.synchronize(dev)

    same = lambda a, c: torch.equal(a.view(torch.int32), c.view(torch.int32))  # noqa: E731
    assert torch.isfinite(out_p).all() and same(out_h, out_p), "descriptors"
    for l in range(7):
        assert torch.isfinite(dws_p[l]).all() and same(dws_h[l], dws_p[l]), f"weight gradient {l}"
        assert same(rm_h[l], rm_p[l]) and same(rv_h[l], rv_p[l]), f"running statistics {l}"
        assert not torch.equal(rm_p[l].cpu(), stats0[l][0]), f"running_mean {l} was updated"
    assert torch.isfinite(din_p).all() and same(din_h, din_p), "input gradient"
