"""What the extension plans share (docs/parity.md, "Plan lifecycle"): the context an inner plan sees, the argument helpers, and ExtPlan,
the host lifecycle of RealFFTPlan, ConvPlan, R2RPlan, FirPlan and HalfFFTPlan -- batch-sized scratch and what becomes of it once a graph
has recorded an execute, the opening and the end of a call, finish / check / close / release_captured over an optional inner plan.

ExtPlan holds plain helpers that a subclass calls in the order ITS execute needs (the orders differ: see each class); it calls nothing
of the subclass back.  GenericFFTPlan owns two work arrays and several inner plans, so it keeps its own _prepare and plan-level
methods and takes only the stateless helpers (upload, stream_step, epilogue, needs_eager_first).  FFTPlan (plan.py) shares
nothing with this module: its state is richer (ring slots, counters, side streams) and its execute is launch-bound.
"""

import numpy

from .passes import is_pow2
from .plan import on_plan_device


class _SubContext(object):
    """What the inner power-of-two plans see: the outer plan's context with the stream choice frozen (the outer execute()
    has already picked the stream of this call; an inner plan must not pick another one)."""

    _guard = False      # the outer plan has made its device current before an inner plan runs

    def __init__(self, ctx):
        self._ctx = ctx
        self.compute_units = ctx.compute_units
        self.machine = ctx.machine
        self.allocate = ctx.allocate
        self.allocate_raw = ctx.allocate_raw
        self.upload = ctx.upload
        self.pointer_of = ctx.pointer_of

    def createQueue(self, buffers=()):
        pass

    def order_scratch(self, capturing=None):
        pass            # (the outer execute() has ordered the stream of this call behind the previous one)

    def stream_handle(self):
        return self._ctx.stream_handle()

    def capturing(self):
        return self._ctx.capturing()

    def wait(self):
        self._ctx.wait()

    def wait_scratch(self):
        self._ctx.wait_scratch()

    def flush(self):
        pass

    def getQueue(self):
        return self._ctx.getQueue()


def pow2_shape(shape, wrong_shape, not_pow2):
    """`shape` (an integer or a tuple of one to three) as a numpy-order tuple of ints, every one a power of two, or a ValueError with
    the caller's text for a malformed shape / for an axis that is not a power of two."""
    if isinstance(shape, (int, numpy.integer)) and not isinstance(shape, bool):
        shape = (shape,)
    if not isinstance(shape, tuple) or not 1 <= len(shape) <= 3:
        raise ValueError(wrong_shape)
    for v in shape:
        if not isinstance(v, (int, numpy.integer)) or isinstance(v, bool) or v < 1:
            raise ValueError(wrong_shape)
    shape = tuple(int(v) for v in shape)
    if not all(is_pow2(v) for v in shape):
        raise ValueError(not_pow2)
    return shape


def buffer_nbytes(obj):
    """Size of a buffer-like object when it knows it (DeviceArray, torch tensor), else None."""
    nb = getattr(obj, "nbytes", None)
    if isinstance(nb, (int, numpy.integer)):
        return int(nb)
    if hasattr(obj, "data_ptr") and hasattr(obj, "numel") and hasattr(obj, "element_size"):
        return int(obj.numel()) * int(obj.element_size())
    return None


def needs_eager_first(call="execute"):
    """The refusal of a call that would allocate on a capturing stream (nothing can be allocated or released inside a capture)."""
    return "pyfft_amd: %s() on a capturing stream needs one eager %s() of the same batch first" % (call, call)


def upload(ctx, host):
    """A host table on the device: the allocation (the plan keeps it; pointer_of gives its address)."""
    host = numpy.ascontiguousarray(host)
    mem = ctx.allocate_raw(host.nbytes)
    ctx.upload(mem, host)
    return mem


def stream_step(plan, capturing):
    """Order the stream of this call behind the plan's previous one; on a capture, the graph bakes in the plan's table and scratch
    addresses: an open hip.Graph keeps the plan alive, the plan keeps what the graph replays on (_captured)."""
    plan._context.order_scratch(capturing)
    if capturing:
        from .hip import Graph
        plan._captured = True
        Graph.retain(plan)


def epilogue(plan, wait):
    """The end of every execute (plan.py:250-259): wait (and check for errors) or hand the stream back."""
    if wait:
        plan.finish()
        return None
    plan._context.flush()
    return plan._context.getQueue()


class ExtPlan(object):
    """Lifecycle state and helpers of an extension plan: see the module docstring.  A subclass sets _inner in its _build where it
    has an inner plan (built on _sub), and keeps a _prepare(batch) of its own over _size_scratch."""

    def __init__(self, context, wait_for_finish):
        self._context = context
        self._wait_for_finish = wait_for_finish
        self._sub = _SubContext(context)
        self._inner = None
        self._scratch = None
        self._last_batch = 0
        self._captured = False
        self._capture_keepalive = []

    def _upload(self, host):
        return upload(self._context, host)

    def _size_scratch(self, batch, nbytes, call="execute"):
        """Plan-owned scratch of `nbytes` for `batch` (None: this form needs none), kept alive for a graph that recorded the previous
        one.  The batch is committed only after the allocation: after a failed one the plan is as close() leaves it."""
        if batch == self._last_batch and (self._scratch is not None or nbytes is None):
            return
        if nbytes is not None and self._context.capturing():
            raise RuntimeError(needs_eager_first(call))
        self._release_scratch()
        if nbytes is not None:
            self._scratch = self._context.allocate(nbytes)
        self._last_batch = batch

    def _release_scratch(self):
        """Let go of the scratch: to the keep-alive list once a graph has recorded an execute (it replays on it); else, where it came
        from a mempool, only after the plan's own asynchronous executes have finished with it (hipFree does that waiting itself)."""
        if self._scratch is not None:
            if self._captured:
                self._capture_keepalive.append(self._scratch)
            else:
                self._context.wait_scratch()
        self._scratch = None
        self._last_batch = 0

    def _open(self, buffers, wait_for_finish=None, call="execute"):
        """Choose the stream of this call; (wait, capturing), or the refusal of a call that would wait on a capturing stream.
        wait_for_finish None: the plan's (filter_spectrum has no per-call one, and says so in its refusal)."""
        ctx = self._context
        ctx.createQueue(buffers)
        wait = self._wait_for_finish if wait_for_finish is None else wait_for_finish
        capturing = ctx.capturing()
        if capturing and wait:
            raise RuntimeError("pyfft_amd: %s() on a capturing stream cannot wait for the result: build the plan with stream=%s" % (
                call, " (or wait_for_finish=False), or pass wait_for_finish=False to this call" if call == "execute" else ""))
        return wait, capturing

    _stream_step = stream_step
    _epilogue = epilogue

    # ------------------------------------------------------------------------------------
    @on_plan_device
    def finish(self):
        """Wait for the plan's stream, then raise if the inner plan reported invalid results."""
        self._context.wait()
        if self._inner is not None:
            self._inner.finish()

    @on_plan_device
    def check(self):
        """Non-blocking: raise if a completed asynchronous execute() of the inner plan reported invalid results."""
        if self._inner is not None:
            self._inner.check()

    def close(self):
        """Wait for outstanding work and release the scratch now; the plan stays usable.  What a recorded graph replays on is kept
        until release_captured()."""
        try:
            self.finish()
        finally:
            self._release_scratch()
            if self._inner is not None:
                self._inner.close()

    def release_captured(self):
        self.finish()
        self._capture_keepalive = []
        self._captured = False
        if self._inner is not None:
            self._inner.release_captured()

    @property
    def inner_plan(self):
        return self._inner
