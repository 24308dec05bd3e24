"""Pipeline.step()'s stream handling: every launch goes to the stream the afm context is bound to
(and that is torch's current stream), the binding is back on the caller's stream after a step
-- also after a step that raised -- and the stage / kernel marks are recorded on every path."""
import ctypes

import pytest

from test_sharded import SPLIT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def grid():
    import torch
    import afm
    from afm.synthetic import make_panel
    torch.cuda.set_device(0)
    return afm.PanelGrid.from_panel(make_panel(300, 700, seed=11, tradable_p=0.9))


class BoundLib:
    """Thin proxy over libafm: remembers the stream of the last afm_ctx_set_stream and checks, at
    every other afm_* call on the context, that it is torch's current stream.  ``fail``: the
    entry point that raises AfmError instead of launching."""

    def __init__(self, real, ctx, fail=None):
        self.real, self.ctx, self.fail = real, ctx, fail
        self.bound, self.launches = None, 0

    def __getattr__(self, name):
        import torch
        from afm._lib import AfmError
        fn = getattr(self.real, name)
        if not name.startswith("afm_"):
            return fn

        def call(*args):
            if name == "afm_ctx_set_stream":
                self.bound = args[1].value or 0
            elif args and isinstance(args[0], ctypes.c_void_p) \
                    and args[0].value == self.ctx.handle.value:
                cur = torch.cuda.current_stream(self.ctx.device).cuda_stream
                assert self.bound == cur, f"{name}: context on {self.bound}, current stream {cur}"
                self.launches += 1
                if name == self.fail:
                    raise AfmError(f"{name}: injected failure (nothing launched)")
            return fn(*args)
        return call


def _proxied(monkeypatch, pipe, fail=None):
    from afm import _lib
    proxy = BoundLib(_lib.lib(), pipe.ctx, fail)
    monkeypatch.setattr(_lib, "lib", lambda: proxy)
    return proxy


# (placement, emulated (world, rank)); rank 7 of 8 is the short last shard -- on 300 assets it is
# empty, so the step takes every "no assets" branch
CASES = [({}, None), ({"zstats_slabs": 0}, None), ({"early_zstats": True, "zstats_slabs": 0}, None),
         ({"labels_side": False}, None), ({}, (2, 0)), ({}, (8, 7))]


def _pipeline(grid, place, emu):
    from afm.pipeline import Pipeline, PipelineConfig
    from afm.sharded import EmulatedComm
    return Pipeline(grid, PipelineConfig(**SPLIT, **place), EmulatedComm(*emu) if emu else None)


@pytest.mark.parametrize("place,emu", CASES)
def test_launches_follow_the_bound_stream(grid, monkeypatch, place, emu):
    import torch
    pipe = _pipeline(grid, place, emu)
    if not place and emu is None:
        assert pipe.stream_z                      # the default on this grid: the streamed path
    if place.get("early_zstats"):
        assert pipe.early
    proxy = _proxied(monkeypatch, pipe)
    pipe.step()
    torch.cuda.synchronize()
    assert proxy.launches > 0                     # the step's launches went through the proxy
    assert proxy.bound == torch.cuda.current_stream(grid.device).cuda_stream


def test_binding_restored_after_a_failed_launch(grid, monkeypatch):
    """A side-stream launch that raises (before anything is launched) leaves neither torch's
    current stream nor the context on the side stream."""
    import torch
    from afm._lib import AfmError
    pipe = _pipeline(grid, {}, None)
    caller = torch.cuda.current_stream(grid.device)
    proxy = _proxied(monkeypatch, pipe, fail="afm_labels_f64")
    with pytest.raises(AfmError, match="injected"):
        pipe.step()
    torch.cuda.synchronize()
    assert torch.cuda.current_stream(grid.device) == caller
    assert proxy.bound == caller.cuda_stream


@pytest.mark.parametrize("place,emu,path", [({"zstats_slabs": 0}, None, "one_pass"),
                                            ({}, None, "streamed"),
                                            ({"early_zstats": True, "zstats_slabs": 0}, None,
                                             "early"),
                                            ({}, (2, 0), "streamed")])
def test_marks_recorded(grid, place, emu, path):
    import torch
    from afm.pipeline import EXCHANGE_STAGES, KERNEL_MARKS, STAGES
    pipe = _pipeline(grid, place, emu)
    assert {"streamed": pipe.stream_z, "early": pipe.early,
            "one_pass": not (pipe.stream_z or pipe.early)}[path]
    stages = EXCHANGE_STAGES if emu else STAGES
    ev = {s: (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
          for s in stages + KERNEL_MARKS}
    pipe.step()
    pipe.step(ev)
    torch.cuda.synchronize()
    ms = {s: ev[s][0].elapsed_time(ev[s][1]) for s in stages}
    assert all(v >= 0 and v == v for v in ms.values()), ms
    k_gram = ev["k_gram"][0].elapsed_time(ev["k_gram"][1])
    assert 0 < k_gram <= ms["xs_gram"]
    if path == "one_pass":
        k_factor = ev["k_factor"][0].elapsed_time(ev["k_factor"][1])
        assert 0 < k_factor <= ms["factors"]


def test_call_refuses_wrong_buffers_before_the_library(monkeypatch):
    """Context.call checks a buffer against the parameter's declared element type: an int64 tensor
    or a strided view where afm_vec_add_f64 takes double* is refused in Python -- the library is
    not entered -- and the well-formed call adds the vectors."""
    import torch
    from afm import _lib
    torch.cuda.set_device(0)
    proxy = BoundLib(_lib.lib(), _lib.Context.get(0))
    monkeypatch.setattr(_lib, "lib", lambda: proxy)
    x = torch.arange(64, dtype=torch.float64, device="cuda")
    y = torch.ones(64, dtype=torch.float64, device="cuda")
    wide = torch.zeros(128, dtype=torch.float64, device="cuda")
    with pytest.raises(_lib.AfmError, match="afm_vec_add_f64 argument 2"):
        _lib.run("afm_vec_add_f64", 64, x.long(), y)
    with pytest.raises(_lib.AfmError, match="afm_vec_add_f64 argument 2"):
        _lib.run("afm_vec_add_f64", 64, wide[::2], y)
    assert proxy.launches == 0
    _lib.run("afm_vec_add_f64", 64, x, y)
    torch.cuda.synchronize()
    assert proxy.launches == 1 and torch.equal(y, x + 1)
