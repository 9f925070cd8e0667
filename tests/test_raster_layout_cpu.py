"""Where the rasteriser's host code lives: _raster_state.py (what is remembered between calls) <- _raster_launch.py (one call
through the C-ABI) <- rasterizer.py (the module every caller imports). The façade re-exports the objects of the two modules under
it — the same objects, no copies and no forwarding functions — and the imports run in that one direction. No GPU, no library."""
import ast
import os

import pytest

from guassianhand_amd import _raster_launch as RL
from guassianhand_amd import _raster_state as RS
from guassianhand_amd import rasterizer as R

# Every name rasterizer.py defined while it was one file (classes, functions, module-level constants and objects), written out so
# that the test does not depend on that file. Not listed: the modules it imported for its own use (ctypes as C, os, threading,
# _abi, _lib, ...): the façade imports what it uses, and nobody reads another module through it.
STATE = ("GhOverflowError", "GhStaleGeometryError", "GhDepthBoundMiss", "DepthBoundCache", "GeometryCache", "_DeviceState", "_Policy",
         "_policy", "_states", "_states_lock", "_dev_index", "_state", "CounterWord", "counter_word", "_learn_depth24", "_grow_capacity",
         "_DEPTH24_MSG", "_STALE_MSG", "_MISS_MSG", "_PENDING_MAX", "_Pending", "last_guard", "last_num_rendered", "enable_stage_timing",
         "set_graph_mode", "graph_counters", "_SPLIT_AUTO_MIN_PIXELS", "set_split_streams", "set_fused_loss", "capacity_key",
         "_initial_capacity", "report_counter_word", "check_overflow", "_WS_POOL_DEPTH", "_ws_acquire", "_ws_release",
         "clear_workspace_pool", "_queue_readback", "_record", "last_grad_block", "set_geometry_reuse")
LAUNCH = ("stage_timing_summary", "_run_stages", "_raw_stream", "_OnDevice", "_ptr", "_prep", "_Ctx", "_Call", "_prepare_call",
          "_inputs_struct", "_fused_loss", "_launch", "_fits_owner", "_forward_shared", "_forward_refresh", "_forward_full",
          "raster_forward", "cached_raster_forward", "raster_backward", "workspace_counters", "workspace_views")
FACADE = ("GaussianRasterizationSettings", "_geometry_key", "_RasterizeGaussians", "_any_global_hook", "GaussianRasterizer", "_ViewArgs",
          "_GRAD_AT", "_GRAD_NAMES", "_apply_views", "_views_forward", "_views_backward", "_RasterizeViews", "rasterize_views",
          "_LEGACY_STATE", "_LEGACY_POLICY")


def test_facade_exposes_every_name_as_the_owning_modules_object():
    assert len(set(STATE + LAUNCH + FACADE)) == len(STATE) + len(LAUNCH) + len(FACADE) == 77
    for owner, names in ((RS, STATE), (RL, LAUNCH)):
        for n in names:
            assert n in vars(owner), f"{owner.__name__} does not define {n}"
            assert getattr(R, n) is vars(owner)[n], f"rasterizer.{n} is not {owner.__name__}.{n}"
            assert getattr(vars(owner)[n], "__module__", owner.__name__) in (owner.__name__, "_thread"), n   # defined there (_thread: the lock)
    for n in FACADE:
        assert n in vars(R), n
        assert getattr(vars(R)[n], "__module__", R.__name__) == R.__name__, n
        assert n not in vars(RS) and n not in vars(RL), n
    # the launch path reads the state's objects, not copies: one policy, one table of device states
    assert RL._policy is RS._policy is R._policy and RL._state is RS._state
    st = RS._DeviceState(96)
    R._states[96] = st
    try:
        assert RS._state(96) is st and R._state(96) is st
        R.check_overflow(dev=96)                                   # (nothing pending: looks at this very object and returns)
        assert st.pending == []
    finally:
        del R._states[96]


def test_legacy_names_resolve_to_the_current_device_and_the_policy():
    st = RS._state()
    for name, attr in R._LEGACY_STATE.items():
        assert getattr(R, name) is getattr(st, attr), name
    for name, attr in R._LEGACY_POLICY.items():
        assert getattr(R, name) is getattr(RS._policy, attr), name
    assert R._split_policy is RS._policy.split and R._capacity is st.capacity
    with pytest.raises(AttributeError):
        R._no_such_attribute


def _imports(module):
    """Last component of every module a file imports, and every name it imports from a package-relative module."""
    with open(os.path.splitext(module.__file__)[0] + ".py") as f:
        tree = ast.parse(f.read())
    found = set()
    for node in ast.walk(tree):
        if isinstance(node, ast.Import):
            found.update(a.name.split(".")[-1] for a in node.names)
            found.update(a.name.split(".")[0] for a in node.names)
        elif isinstance(node, ast.ImportFrom):
            if node.module:
                found.update(node.module.split("."))
            if node.module in (None, "guassianhand_amd"):                 # from . import x / from guassianhand_amd import x
                found.update(a.name for a in node.names)
    return found


def test_imports_run_in_one_direction():
    state, launch = _imports(RS), _imports(RL)
    assert not state & {"ctypes", "_lib", "_call", "camera", "_raster_launch", "rasterizer"}, state
    assert "_abi" in state and "torch" in state
    assert "rasterizer" not in launch and "_raster_state" in launch
