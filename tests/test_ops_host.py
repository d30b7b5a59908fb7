"""Host-side logic of fiber_amd/ops.py that needs no GPU: the one-shot hand-over of column sums from a producing backward
(window attention: the qkv bias gradient) to the linear backward that follows it, and of "the ignored rows are zero" from the cross-entropy
backward to the decoder's; the retired entry points the benchmark still calls."""
import inspect

import pytest
import torch

from fiber_amd import lib, ops


class _Producer(torch.autograd.Function):
    """Stands in for the window-attention backward: returns a gradient and offers `sums` for it."""

    @staticmethod
    def forward(ctx, x, sums, box):
        ctx.sums, ctx.box = sums, box
        return x.clone()

    @staticmethod
    def backward(ctx, dy):
        g = dy.clone()
        ops._offer_colsum(g.view(-1, g.shape[-1]), ctx.sums)
        ctx.box.append(g)
        return g, None, None


class _Consumer(torch.autograd.Function):
    """Stands in for a linear backward: takes the slot for the dY it receives."""

    @staticmethod
    def forward(ctx, x, box):
        ctx.box = box
        return x * 2.0

    @staticmethod
    def backward(ctx, dy):
        ctx.box.append(ops._take_colsum(dy.view(-1, dy.shape[-1])))
        return dy * 2.0, None


def test_colsum_handover_matches_only_the_offered_tensor():
    sums = torch.arange(6.0)
    # producer's gradient flows straight into the consumer: the consumer gets the offered sums
    x = torch.randn(4, 6, requires_grad=True)
    got, grads = [], []
    _Producer.apply(_Consumer.apply(x, got), sums, grads).sum().backward()
    assert len(got) == 1 and got[0] is sums
    assert getattr(ops._hint_tls, "slot", None) is None
    # nobody takes the offer: it does not outlive the autograd pass
    x = torch.randn(4, 6, requires_grad=True)
    _Producer.apply(x, sums, []).sum().backward()
    assert getattr(ops._hint_tls, "slot", None) is None
    # a consumer whose dY is another tensor (different storage) gets nothing and clears the slot
    x = torch.randn(4, 6, requires_grad=True)
    got = []
    y = _Consumer.apply(x, got)
    z = _Producer.apply(y * 1.0, sums, [])          # the multiplication puts a fresh tensor between producer and consumer
    z.sum().backward()
    assert got == [None] and getattr(ops._hint_tls, "slot", None) is None
    # same storage but another shape is not a match either
    t = torch.zeros(4, 6)

    class _Offer(torch.autograd.Function):
        @staticmethod
        def forward(ctx, a):
            return a.clone()

        @staticmethod
        def backward(ctx, dy):
            ops._offer_colsum(t, sums)
            res.append(ops._take_colsum(t.view(2, 12)))
            res.append(ops._take_colsum(t))            # the first take cleared the slot
            return dy

    res = []
    _Offer.apply(torch.randn(3, requires_grad=True)).sum().backward()
    assert res == [None, None]


class _RowsProducer(torch.autograd.Function):
    """Stands in for _CrossEntropy / _SeqLogProb: a gradient whose rows with label == ignore are zero, offered as such."""

    @staticmethod
    def forward(ctx, x, labels, ignore):
        ctx.labels, ctx.ignore = labels, ignore
        return x.sum()

    @staticmethod
    def backward(ctx, g):
        dx = torch.ones(ctx.labels.shape[0], 5) * (ctx.labels != ctx.ignore)[:, None] * g
        ops._offer_labelled_rows(dx, ctx.labels, ctx.ignore)
        return dx, None, None


class _RowsConsumer(torch.autograd.Function):
    """Stands in for _LibLinear: the bias gradient over the labelled rows when the slot says so, else over all rows."""

    @staticmethod
    def forward(ctx, x, b, box):
        ctx.box = box
        return x + b

    @staticmethod
    def backward(ctx, dy):
        hint = ops._take_labelled_rows(dy)
        ctx.box.append(hint)
        db = dy[hint[0] != hint[1]].sum(0) if hint is not None else dy.sum(0)
        return dy, db, None


def _slot(tls):
    return getattr(tls, "slot", None)


def test_labelled_rows_offer_does_not_outlive_its_backward_pass():
    lab = torch.tensor([3, -100, -100, 1, -100, -100])
    # taken by the consumer it was meant for: used, and gone
    x, b, box = torch.randn(6, 5, requires_grad=True), torch.zeros(5, requires_grad=True), []
    _RowsProducer.apply(_RowsConsumer.apply(x, b, box), lab, -100).backward()
    assert box[0] is not None and box[0][0] is lab and box[0][1] == -100
    assert torch.equal(b.grad, torch.full((5,), 2.0)) and _slot(ops._rows_tls) is None
    # nobody takes it (the logits are a leaf): the end of the pass clears it
    leaf = torch.randn(6, 5, requires_grad=True)
    _RowsProducer.apply(leaf, lab, -100).backward()
    assert _slot(ops._rows_tls) is None
    # ... also when the pass runs twice on a retained graph
    loss = _RowsProducer.apply(leaf, lab, -100)
    loss.backward(retain_graph=True)
    assert _slot(ops._rows_tls) is None
    loss.backward()
    assert _slot(ops._rows_tls) is None


def test_labelled_rows_stale_offer_is_not_matched_by_a_later_pass():
    """(g) of tests/test_hip_autograd_graphs.py with stand-ins: the producer's dx becomes a leaf's .grad, the caller writes into its ignored
    rows and feeds it to a consumer of the same shape in ANOTHER pass: the bias gradient is the sum over all rows."""
    lab = torch.tensor([3, -100, -100, 1, -100, -100])
    leaf = torch.randn(6, 5, requires_grad=True)
    _RowsProducer.apply(leaf, lab, -100).backward()
    leaf.grad[lab == -100] += 0.5
    x, b, box = torch.randn(6, 5, requires_grad=True), torch.zeros(5, requires_grad=True), []
    _RowsConsumer.apply(x, b, box).backward(gradient=leaf.grad)
    assert box == [None]
    assert torch.equal(b.grad, leaf.grad.sum(0)) and float(b.grad[0]) == 4.0
    assert _slot(ops._rows_tls) is None


def test_in_place_write_between_offer_and_take_voids_both_slots():
    """Address and shape still match after an in-place write (autograd's fan-in add, `grad[...] +=`): the version counter does not."""
    lab, sums = torch.tensor([0, -100, 2]), torch.arange(4.0)
    res = []

    class _Pass(torch.autograd.Function):
        @staticmethod
        def forward(ctx, a, touch):
            ctx.touch = touch
            return a.clone()

        @staticmethod
        def backward(ctx, dy):
            t = torch.zeros(3, 4)
            ops._offer_labelled_rows(t, lab, -100)
            ops._offer_colsum(t, sums)
            if ctx.touch:
                t.view(-1)[1:3] += 1.0                      # through a view: views share the counter
            res.append((ops._take_labelled_rows(t), ops._take_colsum(t.view(3, 4))))
            return dy, None

    for touch in (False, True):
        _Pass.apply(torch.randn(3, requires_grad=True), touch).sum().backward()
    assert res[0][0] is not None and res[0][0][0] is lab and res[0][1] is sums
    assert res[1] == (None, None)
    assert _slot(ops._rows_tls) is None and _slot(ops._hint_tls) is None


def test_fan_in_accumulation_voids_the_offer_whatever_the_construction_order():
    """The offered tensor's other consumer: when its node is created BEFORE the producer's, the producer's backward runs first and autograd
    adds the other gradient into the offered tensor in place (same address, non-zero "ignored" rows).  The consumer must sum all rows."""
    lab = torch.tensor([3, -100, -100, 1, -100, -100])
    for aux_first in (True, False):
        x, b, box = torch.randn(6, 5, requires_grad=True), torch.zeros(5, requires_grad=True), []
        y = _RowsConsumer.apply(x, b, box)
        if aux_first:
            aux = (y * 0.25).sum()
            loss = aux + _RowsProducer.apply(y, lab, -100)
        else:
            loss = _RowsProducer.apply(y, lab, -100)
            loss = loss + (y * 0.25).sum()
        loss.backward()
        assert box == [None], aux_first
        assert torch.equal(b.grad, torch.full((5,), 2.0 + 6 * 0.25))
        assert _slot(ops._rows_tls) is None


def test_retired_wgrad_entry_points_do_nothing_and_touch_no_device():
    """bench.py still calls the switches of the two retired weight-gradient experiments (profiles/wgrad_experiments_retired.md): they
    return without initialising CUDA, switching the stream experiment ON is an error, and ops.wgrad() has no `post` left."""
    before = torch.cuda.is_initialized()
    assert ops.set_fold_defer(True) is None
    assert ops.enable_wgrad_stream(torch.nn.Linear(8, 8)) is False
    assert ops.set_wgrad_stream(False) is None
    assert torch.cuda.is_initialized() == before
    with pytest.raises(lib.FiberHipError):
        ops.set_wgrad_stream(True)
    assert torch.cuda.is_initialized() == before
    assert "post" not in inspect.signature(ops.wgrad).parameters
