"""One pose head (csrc/pose_head.hip behind islam_amd/pose_head.py::PoseHeadHip, or one workspace behind the C ABI) serving a SEQUENCE of
calls: other batch sizes, other spatial sizes, accumulate = 1, frozen parameters, gradients that are already there, parameters that moved.

Reference: the kernels sum in a fixed order (tests/test_pose_head_gpu.py asserts bit-identical repeats), so "the reused head is right"
means "it gives, bit for bit, what a FRESH PoseHeadHip on the same parameters and the same input gives" -- torch.equal on the (B,6)
output and on all 120 parameter gradients.  What a fresh head computes is held against float64 in tests/test_pose_head_gpu.py."""
import ctypes
import gc

import pytest
import torch

pytestmark = pytest.mark.gpu

N_PARAMS = 120


def _net(cuda, seed):
    from islam_amd import nets
    torch.manual_seed(seed)
    return nets.VOFlowRes().to(cuda).to(memory_format=torch.channels_last)


def _inputs(cuda, B, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, 4, H, W, generator=g).to(cuda).contiguous(memory_format=torch.channels_last)
    return x, torch.randn(B, 6, generator=g).to(cuda)


def _step(head, x, gy):
    """Forward and backward from empty .grad: (output, the 120 gradients), both copied."""
    params = list(head.module.parameters())
    for p in params:
        p.grad = None
    y = head(x)
    y.backward(gy)
    return y.detach().clone(), [None if p.grad is None else p.grad.detach().clone() for p in params]


def _fresh(net, x, gy):
    """The reference: (output, gradients) of a fresh head on net and x; the net's .grad fields are put back as they were."""
    from islam_amd import pose_head
    params = list(net.parameters())
    keep = [p.grad for p in params]
    out = _step(pose_head.PoseHeadHip(net), x, gy)
    for p, k in zip(params, keep):
        p.grad = k
    return out


def _assert_same(got, want, what):
    names = [n for n, _ in what.named_parameters()]
    assert torch.equal(got[0], want[0]), 'output'
    bad = [n for n, a, b in zip(names, got[1], want[1]) if a is None or not torch.equal(a, b)]
    assert not bad, '%d of %d gradients differ from a fresh head: %s' % (len(bad), len(names), bad[:8])


def _run_sequence(cuda, shapes, graphs, seed):
    from islam_amd import pose_head
    net = _net(cuda, seed)
    head = pose_head.PoseHeadHip(net, graphs=graphs)
    for i, (B, H, W) in enumerate(shapes):
        x, gy = _inputs(cuda, B, H, W, 1000 * seed + i)
        want = _fresh(net, x, gy)
        if graphs:
            torch.cuda.synchronize()                     # the head drops the graphs of the previous shape: with the device idle
        got = _step(head, x, gy)
        _assert_same(got, want, net)
    torch.cuda.synchronize()
    del head
    gc.collect()
    torch.cuda.synchronize()


@pytest.mark.parametrize('graphs', [False, True])
def test_batch_shrinks_and_grows_on_one_head(cuda, graphs):
    """B = 8 -> 3 -> 8 -> 1 at 112 x 160 (the smaller last batch of an epoch).  The workspace of the B = 8 call is kept; where the plan of
    a smaller batch puts its split-K ticket words the larger one must not have left anything but zeros -- a ticket that starts off
    zero has no last arriver and the tile's epilogue never runs (stale outputs and gradients, no error)."""
    _run_sequence(cuda, [(8, 112, 160), (3, 112, 160), (8, 112, 160), (1, 112, 160)], graphs, seed=21)


def test_spatial_size_changes_on_one_head(cuda):
    """B = 2 at 128 x 192 (the largest served size) -> 65 x 129 (the smallest) -> 100 x 132 -> 128 x 192 on one head."""
    _run_sequence(cuda, [(2, 128, 192), (2, 65, 129), (2, 100, 132), (2, 128, 192)], False, seed=22)


# ---- the C ABI, called directly
def _grad_buffers(params, fill):
    """One flat buffer and one view per parameter in the parameter's own memory layout (as PoseHeadHip._views lays them out)."""
    offs, total = [], 0
    for p in params:
        offs.append(total)
        total += (p.numel() + 63) // 64 * 64
    flat = fill(total)
    views = []
    for p, o in zip(params, offs):
        v = flat[o:o + p.numel()]
        if p.dim() == 4:
            O, I, kh, kw = p.shape
            v = v.view(O, kh, kw, I).permute(0, 3, 1, 2)
        else:
            v = v.view(p.shape)
        views.append(v)
    return flat, views


class _Abi:
    def __init__(self, net, ws):
        from islam_amd import _lib
        self._lib, self.L = _lib, _lib.lib()
        self.params = list(net.parameters())
        assert len(self.params) == N_PARAMS
        self.ptab = (ctypes.c_void_p * N_PARAMS)(*[p.data_ptr() for p in self.params])
        self.ws = ws

    def forward(self, x):
        B, _, H, W = x.shape
        out = torch.empty(B, 6, dtype=torch.float32, device=x.device)
        self._lib.check(self.L.islam_pose_head_forward(ctypes.c_void_p(x.data_ptr()), ctypes.cast(self.ptab, ctypes.c_void_p),
                                                       ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(self.ws.data_ptr()),
                                                       ctypes.c_size_t(self.ws.numel() * 4), B, H, W, self._lib.stream_ptr(x.device)))
        return out

    def backward(self, x, gy, views, accumulate):
        B, _, H, W = x.shape
        gtab = (ctypes.c_void_p * N_PARAMS)(*[v.data_ptr() for v in views])
        self._lib.check(self.L.islam_pose_head_backward(ctypes.c_void_p(x.data_ptr()), ctypes.cast(self.ptab, ctypes.c_void_p),
                                                        ctypes.cast(gtab, ctypes.c_void_p), ctypes.c_void_p(gy.data_ptr()),
                                                        ctypes.c_void_p(self.ws.data_ptr()), ctypes.c_size_t(self.ws.numel() * 4), B, H, W,
                                                        int(accumulate), self._lib.stream_ptr(x.device)))


def _workspace(cuda, B, H, W):
    from islam_amd import _lib
    nbytes = int(_lib.lib().islam_pose_head_workspace_bytes(B, H, W))
    assert nbytes > 0 and nbytes % 4 == 0
    return torch.zeros(nbytes // 4, dtype=torch.float32, device=cuda)


def test_c_abi_one_zero_filled_workspace_serves_several_shapes(cuda):
    """include/islam_hip.h: one workspace, zero-filled ONCE, of the size of the largest call; every call is given the whole buffer."""
    net = _net(cuda, 23)
    abi = _Abi(net, _workspace(cuda, 8, 112, 160))
    for i, (B, H, W) in enumerate([(8, 112, 160), (3, 112, 160), (2, 65, 129)]):
        x, gy = _inputs(cuda, B, H, W, 23000 + i)
        want = _fresh(net, x, gy)
        y = abi.forward(x)
        _, views = _grad_buffers(abi.params, lambda n: torch.zeros(n, dtype=torch.float32, device=cuda))
        abi.backward(x, gy, views, 0)
        _assert_same((y, views), want, net)


def test_c_abi_accumulate_flag(cuda):
    """accumulate = 0 writes EVERY element of every gradient (buffers pre-filled with NaN; the first layer's Cin = 4 weight has an
    epilogue of its own); accumulate = 1 adds to what is there: *dst + v in fp32, one rounding, so the result is bit-equal to G0 + g."""
    B, H, W = 2, 65, 129
    net = _net(cuda, 24)
    x, gy = _inputs(cuda, B, H, W, 24000)
    _, g = _fresh(net, x, gy)
    abi = _Abi(net, _workspace(cuda, B, H, W))
    names = [n for n, _ in net.named_parameters()]
    abi.forward(x)
    _, views = _grad_buffers(abi.params, lambda n: torch.full((n,), float('nan'), dtype=torch.float32, device=cuda))
    abi.backward(x, gy, views, 0)
    unwritten = [n for n, v in zip(names, views) if bool(torch.isnan(v).any())]
    assert not unwritten, unwritten
    assert not [n for n, v, r in zip(names, views, g) if not torch.equal(v, r)]
    gen = torch.Generator().manual_seed(24001)
    _, views = _grad_buffers(abi.params, lambda n: torch.randn(n, generator=gen).to(cuda))
    g0 = [v.clone() for v in views]
    abi.backward(x, gy, views, 1)
    once = [a + b for a, b in zip(g0, g)]
    assert not [n for n, v, r in zip(names, views, once) if not torch.equal(v, r)]
    abi.backward(x, gy, views, 1)
    assert not [n for n, v, r, b in zip(names, views, once, g) if not torch.equal(v, r + b)]


# ---- PoseHeadHip._accumulate
def test_frozen_parameters_get_no_gradient(cuda):
    from islam_amd import pose_head
    net = _net(cuda, 25)
    x, gy = _inputs(cuda, 2, 65, 129, 25000)
    _, want = _fresh(net, x, gy)
    for p in net.voflow_rot.parameters():
        p.requires_grad_(False)
    frozen = {id(p) for p in net.voflow_rot.parameters()}
    assert len(frozen) == 6
    head = pose_head.PoseHeadHip(net)
    for rep in range(2):                                 # second step: onto the gradients of the first
        y = head(x)
        y.backward(gy)
        for (n, p), w in zip(net.named_parameters(), want):
            if id(p) in frozen:
                assert p.grad is None, n
            else:
                assert torch.equal(p.grad, w if rep == 0 else w + w), n


def test_gradients_of_an_eager_backward_are_added_to(cuda):
    from islam_amd import pose_head
    net = _net(cuda, 26)
    x, gy = _inputs(cuda, 2, 65, 129, 26000)
    _, g = _fresh(net, x, gy)
    net(x).backward(gy)                                  # the module's eager path: AccumulateGrad leaves its own tensors in .grad
    eager = [p.grad.detach().clone() for p in net.parameters()]
    head = pose_head.PoseHeadHip(net)
    head(x).backward(gy)
    for (n, p), e, w in zip(net.named_parameters(), eager, g):
        assert torch.equal(p.grad, e + w), n


def test_flat_accumulation_follows_zero_grad_and_moved_parameters(cuda):
    """The one-launch path (every .grad a view of one flat buffer): across optimizer.zero_grad(set_to_none=False / True), and after the
    parameters' storage was rebuilt (other data pointers: the head builds its tables again)."""
    from islam_amd import pose_head
    net = _net(cuda, 27)
    x, gy = _inputs(cuda, 2, 65, 129, 27000)
    opt = torch.optim.SGD(net.parameters(), lr=1e-3)
    head = pose_head.PoseHeadHip(net)

    def step_and_check(reps):
        _, want = _fresh(net, x, gy)
        for rep in range(1, reps + 1):
            head(x).backward(gy)
            for (n, p), w in zip(net.named_parameters(), want):
                acc = w
                for _ in range(rep - 1):
                    acc = acc + w
                assert torch.equal(p.grad, acc), (n, rep)

    step_and_check(2)                                    # .grad None -> the flat buffer; then flat += flat
    assert head.acc_flat is not None and all(p.grad.data_ptr() == a.data_ptr() for p, a in zip(net.parameters(), head.acc_views))
    opt.step()
    opt.zero_grad(set_to_none=False)                     # zeros in place: .grad stays the head's views
    assert all(p.grad.data_ptr() == a.data_ptr() for p, a in zip(net.parameters(), head.acc_views))
    step_and_check(2)
    opt.step()
    opt.zero_grad(set_to_none=True)
    step_and_check(2)
    # rebuild the parameter storage: every convolution weight gets new memory
    opt.zero_grad(set_to_none=True)
    before = [p.data_ptr() for p in net.parameters()]
    net.to(memory_format=torch.contiguous_format)
    net.to(memory_format=torch.channels_last)
    assert any(a != p.data_ptr() for a, p in zip(before, net.parameters()))
    step_and_check(2)

