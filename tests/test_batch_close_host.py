"""device.Batch.close after its context is gone, without a GPU.

cpr_batch_destroy reads the batch's context, which cpr_ctx_destroy frees. A batch that a
failed test left unclosed reached the garbage collector after the module's context fixture
had closed the context, and the run ended in a segmentation fault instead of the failure's
report. The wrapper drops such a batch without the call.
"""

from cpr_amd import _lib as L
from cpr_amd import device


class _Ctx:
    def __init__(self, handle):
        self.handle = handle


class _Lib:
    def __init__(self):
        self.destroyed = []

    def cpr_batch_destroy(self, h):
        self.destroyed.append(h)


def _batch(ctx_handle):
    b = device.Batch.__new__(device.Batch)
    b.ctx = _Ctx(ctx_handle)
    b.handle = 0xB47C4
    return b


def test_close_destroys_once_while_the_context_lives(monkeypatch):
    fake = _Lib()
    monkeypatch.setattr(L, "lib", lambda: fake)
    b = _batch(0xC0)
    b.close()
    b.close()
    assert fake.destroyed == [0xB47C4] and b.handle is None


def test_close_after_the_context_makes_no_call(monkeypatch):
    fake = _Lib()
    monkeypatch.setattr(L, "lib", lambda: fake)
    b = _batch(None)  # Context.close() leaves handle None
    b.close()
    assert fake.destroyed == [] and b.handle is None
    del b  # __del__ goes through close
    assert fake.destroyed == []
