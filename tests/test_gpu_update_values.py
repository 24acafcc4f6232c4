"""irt_update_values / irt_update_values_device / irt_update_values_end: a scene's value[] replaced
in place (the next step of a time series) leaves the context indistinguishable from a fresh one
created from the same records with the new values -- the yardstick of every test here -- bit for
bit: the blocks, the shell, the volume facts, the grid, frames and their counts.

Scenes: the smallest that reach every branch of the shell rebuild -- flat (sorted heights: the
running findHeight index) and terrain (inverted first layers: the literal search; zero-thickness
top records; voids); both hold the antimeridian and polar rectangles of the wide-rectangle path.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import irt
from helpers import bits, oracle_frame

pytestmark = pytest.mark.gpu

W = 96
SETS = "ABCD"


@functools.lru_cache(maxsize=None)
def scene(name):
    cells = irt.synth_grid(2, 1, 45) if name == "flat" else irt.synth_grid(2, 2, 65, terrain=4000)
    cells.setflags(write=False)
    return cells


@functools.lru_cache(maxsize=None)
def values(name, which):
    """The value sets, (n, 32) float32, from the scene's own values."""
    cells = scene(name)
    v = cells["value"].astype(np.float32)
    if which == "A":
        out = np.float32(1) - v
    elif which == "B":  # narrower: stale minima / maxima would survive a shell not re-initialised
        out = np.float32(0.25) + np.float32(0.5) * v
    elif which == "C":  # wider: leaves the transfer function's range on both sides
        out = np.float32(3) * v - np.float32(1)
    else:  # random, with distinct junk in the slots numLayers..31
        rng = np.random.default_rng(5)
        out = rng.random(v.shape, dtype=np.float32)
        junk = (100 + np.arange(v.size, dtype=np.float32)).reshape(v.shape)
        unused = np.arange(32)[None, :] >= cells["numLayers"][:, None]
        out[unused] = junk[unused]
    out = np.ascontiguousarray(out, dtype=np.float32)
    out.setflags(write=False)
    return out


def with_values(cells, vals):
    out = np.array(cells, copy=True)
    out["value"] = vals
    return out


@functools.lru_cache(maxsize=None)
def setup(name):
    """The frame setup of the scene as created: camera, default transfer function over the
    original data range (the caller's: updates leave it alone)."""
    return irt.setup_frame(scene(name), W, W)


def new_context(cells, name):
    ctx = irt.Context(cells, 0)
    s = setup(name)
    ctx.set_transfunc(s.lut, s.value_range)
    return ctx


@functools.lru_cache(maxsize=None)
def fresh(name, which):
    """The yardstick: a context created from the records with the value set in place (None: the
    scene as it is), with the scene's transfer function.  Shared, never updated."""
    cells = scene(name) if which is None else with_values(scene(name), values(name, which))
    return new_context(cells, name)


def frame(ctx, name, raygen=0, frames=1, accel=0, mode=0, stream=0):
    import torch
    s = setup(name)
    lp = irt.LaunchParams.from_buffer_copy(s.lp)
    lp.raygen, lp.accelMode, lp.mode, lp.accumID = raygen, accel, mode, 0
    fb = torch.zeros(W * W, dtype=torch.int32, device="cuda")
    acc = torch.zeros(W * W * 4, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    if frames == 1:
        ctx.render(lp, W, W, fb.data_ptr(), acc.data_ptr(), stream)
    else:
        ctx.render_accumulate(lp, W, W, frames, fb.data_ptr(), acc.data_ptr(), stream)
    torch.cuda.synchronize()
    st = ctx.stats()
    return fb.cpu().numpy().copy(), bits(acc.cpu().numpy()), (st.locateCalls, st.samplesFound, st.raysInBox)


def assert_same_frame(got, ref, what):
    assert np.array_equal(got[1], ref[1]), f"{what}: accum differs"
    assert np.array_equal(got[0], ref[0]), f"{what}: fb differs"
    assert got[2] == ref[2], f"{what}: counts {got[2]} vs {ref[2]}"


def assert_same_arrays(ctx, ref, what):
    assert np.array_equal(ctx.array("blocks"), ref.array("blocks")), f"{what}: blocks"
    (vr, mo), (rvr, rmo) = ctx.shell(), ref.shell()
    assert np.array_equal(bits(vr), bits(rvr)), f"{what}: shell ranges"
    assert np.array_equal(bits(mo), bits(rmo)), f"{what}: shell majorants"
    assert bytes(ctx.info)[:-8] == bytes(ref.info)[:-8], f"{what}: volume info"  # all but deviceBytes


KEPT = ("fat", "bin_hdr", "sph_r", "sph_off", "sph_rec", "sph_bits")


# ------------------------------------------------------------------ 1. arrays
@pytest.mark.parametrize("name", ["flat", "terrain"])
def test_arrays_equal_a_fresh_context(name):
    ctx = new_context(scene(name), name)
    kept = {k: ctx.array(k).copy() for k in KEPT}
    for which in SETS:  # in sequence on the same context
        ctx.update_values(values(name, which))
        ctx.end_update()
        assert_same_arrays(ctx, fresh(name, which), f"{name} ({which})")
        for k in KEPT:
            assert np.array_equal(ctx.array(k), kept[k]), f"{name} ({which}): {k} changed"
    ctx.close()


# ------------------------------------------------------------------ 2. chunking
@pytest.mark.parametrize("name", ["flat", "terrain"])
def test_chunks_in_any_order(name):
    import torch
    ctx = new_context(scene(name), name)
    D = values(name, "D")
    n = D.shape[0]
    bounds = [(0, 1), (1, 256), (256, 513), (513, n)]
    for lo, hi in reversed(bounds):
        ctx.update_values(np.ascontiguousarray(D[lo:hi]), first=lo)
    ctx.end_update()
    assert_same_arrays(ctx, fresh(name, "D"), f"{name}: chunks, reversed")
    # ... and from device memory, one chunk of it through a pointer that is only 4-B aligned
    ctx.update_values(values(name, "A"))
    flat = torch.zeros(1 + D.size, dtype=torch.float32, device="cuda")
    flat[1:] = torch.from_numpy(np.array(D)).cuda().flatten()
    torch.cuda.synchronize()
    for lo, hi in bounds:
        ctx.update_values_device(flat.data_ptr() + 4 * (1 + 32 * lo), hi - lo, first=lo)
    ctx.end_update()
    assert_same_arrays(ctx, fresh(name, "D"), f"{name}: device chunks")
    ctx.update_values(D)  # once more, as one call
    ctx.end_update()
    assert_same_arrays(ctx, fresh(name, "D"), f"{name}: one call")
    ctx.close()


def test_partial_update_leaves_the_other_records():
    name = "terrain"
    ctx = new_context(scene(name), name)
    mixed = np.array(scene(name)["value"], copy=True)
    mixed[100:357] = values(name, "A")[100:357]
    ctx.update_values(np.ascontiguousarray(values(name, "A")[100:357]), first=100)
    ctx.end_update()
    ref = new_context(with_values(scene(name), mixed), name)
    assert_same_arrays(ctx, ref, "records [100, 357)")
    ctx.close()
    ref.close()


# ------------------------------------------------------------------ 3. frames
@pytest.mark.parametrize("name", ["flat", "terrain"])
def test_frames_equal_a_fresh_context(name):
    ctx = new_context(scene(name), name)
    for which in SETS:
        ctx.update_values(values(name, which))
        ctx.end_update()
        ref = fresh(name, which)
        for raygen in (irt.RAYGEN_WITH_ACCEL, irt.RAYGEN_AE):
            assert_same_frame(frame(ctx, name, raygen), frame(ref, name, raygen), f"{name} ({which}) raygen {raygen}")
        assert_same_frame(frame(ctx, name, frames=8), frame(ref, name, frames=8), f"{name} ({which}) 8 frames")
        assert ctx.chain_errors() == 0 and ref.chain_errors() == 0
    ctx.close()


def test_updated_frame_equals_the_oracle():
    """The fresh-context yardstick is not the only witness: (A) on the terrain scene against the
    CPU oracle, as tests/test_gpu_parity.py compares frames."""
    name = "terrain"
    s = setup(name)
    cells = with_values(scene(name), values(name, "A"))
    a_ref, f_ref, st_ref, _ = oracle_frame(cells, W, W, lut=s.lut, value_range=s.value_range)
    ctx = new_context(scene(name), name)
    ctx.update_values(values(name, "A"))
    ctx.end_update()
    fb, acc, counts = frame(ctx, name)
    assert np.array_equal(acc.reshape(W, W, 4), bits(a_ref)) and np.array_equal(fb.view(np.uint32).reshape(W, W), f_ref)
    assert counts == (st_ref[0].locate_calls, st_ref[0].samples_found, st_ref[0].rays_in_box)
    ctx.close()


# ------------------------------------------------------------------ 4. modes
def test_grid_mode():
    name = "flat"
    ctx = new_context(scene(name), name)
    for which in ("A", "D"):  # before the grid's first use, and after it
        ctx.update_values(values(name, which))
        ctx.end_update()
        ref = fresh(name, which)
        (vr, mo), (rvr, rmo) = ctx.grid(), ref.grid()
        assert np.array_equal(bits(vr), bits(rvr)) and np.array_equal(bits(mo), bits(rmo)), which
        assert_same_frame(frame(ctx, name, accel=irt.ACCEL_GRID), frame(ref, name, accel=irt.ACCEL_GRID),
                          f"grid ({which})")
    ctx.close()


def test_cubql_mode():
    name = "terrain"
    ctx = new_context(scene(name), name)
    ctx.build_wedge_accel(scene(name))
    ctx.update_values(values(name, "A"))
    ctx.end_update()
    ref = new_context(with_values(scene(name), values(name, "A")), name)
    ref.build_wedge_accel(with_values(scene(name), values(name, "A")))
    assert_same_frame(frame(ctx, name, mode=irt.MODE_CUBQL), frame(ref, name, mode=irt.MODE_CUBQL), "CUBQL")
    ctx.close()
    ref.close()


# ------------------------------------------------------------------ 5. transfer function state
def test_update_before_any_transfer_function():
    name = "flat"
    ctx = irt.Context(scene(name), 0)
    ctx.update_values(values(name, "B"))
    ctx.end_update()
    vr, mo = ctx.shell()
    assert not mo.any()
    assert np.array_equal(bits(vr), bits(fresh(name, "B").shell()[0]))
    ctx.close()


# tfSamples is k_accept_stat's sum over count.  The count is exact; the sum is one double
# atomicAdd per workgroup (1024 x 1024 macrocells / 256 = 4096 of them) in whatever order the
# workgroups finish, so two contexts with the same shell -- two fresh ones included -- differ by
# the order's rounding: at most 4096 x 2^-53 of the (all-positive) sum each.  Measured on the flat
# scene: 34.94178772782154 against 34.941787727821456 (2.4e-15 relative).
TF_SAMPLES_REL = 2 * 4096 * 2.0 ** -53


def test_sparse_transfer_function_decision(monkeypatch):
    """The sparse-TF decision (irt_debug_slot_use) equals the fresh context's; tfSamples equals it
    to the rounding of its atomic sum's order (TF_SAMPLES_REL), which is all two runs of
    k_accept_stat over the same shell agree to."""
    monkeypatch.delenv("IRT_SLOTS", raising=False)
    monkeypatch.delenv("IRT_SLOT_SUBS", raising=False)
    name = "flat"
    s = setup(name)
    comb = np.array(s.lut, dtype=np.float32, copy=True)  # tests/test_gpu_slots.py _comb
    comb[:, 3] = 0.01
    comb[::50, 3] = 1.0
    L = irt.lib()
    L.irt_debug_slot_use.argtypes = [C.c_void_p, C.c_void_p]
    ctx = irt.Context(scene(name), 0)
    ctx.set_transfunc(comb, s.value_range)
    for which in ("A", "C"):
        ctx.update_values(values(name, which))
        ctx.end_update()
        ref = irt.Context(with_values(scene(name), values(name, which)), 0)
        ref.set_transfunc(comb, s.value_range)
        got, want = C.c_double(), C.c_double()
        assert L.irt_debug_slot_use(ctx._h, C.byref(got)) == L.irt_debug_slot_use(ref._h, C.byref(want)), which
        print(f"({which}) tfSamples {got.value!r} updated, {want.value!r} fresh")
        assert want.value > 0 and abs(got.value - want.value) <= TF_SAMPLES_REL * want.value, (which, got.value, want.value)
        assert_same_frame(frame(ctx, name), frame(ref, name), f"comb ({which})")
        ref.close()
    ctx.close()


# ------------------------------------------------------------------ 6. device pointer, ordering
def test_device_pointer_on_another_stream():
    import torch
    name = "flat"
    s = setup(name)
    ctx = new_context(scene(name), name)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    A = torch.from_numpy(np.array(values(name, "A"))).cuda()
    bufs = [(torch.zeros(W * W, dtype=torch.int32, device="cuda"),
             torch.zeros(W * W * 4, dtype=torch.float32, device="cuda")) for _ in range(2)]
    torch.cuda.synchronize()
    lp = irt.LaunchParams.from_buffer_copy(s.lp)
    ctx.render(lp, W, W, bufs[0][0].data_ptr(), bufs[0][1].data_ptr(), s1.cuda_stream)
    # no host synchronisation: the update orders itself behind the frame in flight
    ctx.update_values_device(A.data_ptr(), A.shape[0], 0, s2.cuda_stream)
    ctx.end_update()
    ctx.render(lp, W, W, bufs[1][0].data_ptr(), bufs[1][1].data_ptr(), s1.cuda_stream)
    torch.cuda.synchronize()
    for (fb, acc), which in zip(bufs, (None, "A")):
        ref = frame(fresh(name, which), name)
        assert np.array_equal(bits(acc.cpu().numpy()), ref[1]), which
        assert np.array_equal(fb.cpu().numpy(), ref[0]), which
    assert ctx.info.dataRange.lower == fresh(name, "A").info.dataRange.lower
    ctx.close()


# ------------------------------------------------------------------ 7. pending, errors
def test_pending_update_and_argument_errors():
    import torch
    name = "flat"
    s = setup(name)
    ctx = new_context(scene(name), name)
    n = scene(name).size
    fb = torch.zeros(W * W, dtype=torch.int32, device="cuda")
    acc = torch.zeros(W * W * 4, dtype=torch.float32, device="cuda")
    ctx.end_update()  # nothing pending: nothing happens
    assert_same_arrays(ctx, fresh(name, None), "no-op end")
    before = ctx.array("blocks").copy()
    for first, m in ((n, 1), (n - 1, 2), (2 ** 64 - 1, 2)):
        with pytest.raises(irt.IrtError) as e:
            ctx.update_values(np.zeros((m, 32), np.float32), first=first)
        assert e.value.code == irt.E_INVALID
    with pytest.raises(irt.IrtError) as e:
        ctx.update_values_device(0, 4)
    assert e.value.code == irt.E_INVALID
    ctx.render(s.lp, W, W, fb.data_ptr(), acc.data_ptr())  # none of those left an update pending
    assert np.array_equal(ctx.array("blocks"), before)
    ctx.update_values(values(name, "A")[:7])
    for call in (lambda: ctx.render(s.lp, W, W, fb.data_ptr(), acc.data_ptr()),
                 lambda: ctx.render_accumulate(s.lp, W, W, 2, fb.data_ptr(), acc.data_ptr()),
                 lambda: ctx.shell(), lambda: ctx.grid(),
                 lambda: ctx.set_transfunc(s.lut, s.value_range)):
        with pytest.raises(irt.IrtError) as e:
            call()
        assert e.value.code == irt.E_INVALID and "update is pending" in str(e.value)
    ctx.update_values(values(name, "A")[7:], first=7)
    ctx.end_update()
    ctx.set_transfunc(s.lut, s.value_range)
    assert_same_arrays(ctx, fresh(name, "A"), "after the commit")
    assert_same_frame(frame(ctx, name), frame(fresh(name, "A"), name), "after the commit")
    ctx.close()


# ------------------------------------------------------------------ 8. empty and tiny
def test_empty_and_single_record():
    ctx = irt.Context(np.zeros(0, irt.CELL_DTYPE), 0)
    ctx.update_values(np.zeros((0, 32), np.float32))
    ctx.end_update()
    assert bytes(ctx.info)[:-8] == bytes(irt.Context(np.zeros(0, irt.CELL_DTYPE), 0).info)[:-8]
    ctx.close()
    one = np.array(scene("flat")[:1], copy=True)
    vals = np.ascontiguousarray(values("flat", "D")[:1])
    ctx, ref = irt.Context(one, 0), irt.Context(with_values(one, vals), 0)
    ctx.update_values(vals)
    ctx.end_update()
    assert_same_arrays(ctx, ref, "one record")
    ctx.close()
    ref.close()
