"""Progressive render sessions of a RayTracer (gi_progressive_*) with their checkpoint header, and groups of devices (gi_group_*)."""
import ctypes as C
import struct

import numpy as np

from ._abi import GI_E_STATE, GI_OK, GiError, _dev, _ip, _out, _p, lib
from .params import lens_params

# The header of a progressive checkpoint (include/gi_hip.h: gi_progressive_save), little-endian, 192 bytes; the 72-byte pixel records follow.
CHECKPOINT_MAGIC = b"GIPROGR\0"
CHECKPOINT_VERSION = 1
CHECKPOINT_HEADER = "<8sII11d7i4xdQiiQIIiiiI"
CHECKPOINT_RECORD_BYTES = 72
_CHECKPOINT_FIELDS = ("width", "height", "stripe_h", "stripe_rank", "stripe_world", "min_samples", "max_samples", "noise_thresh", "seed",
                      "schedule", "sample_end", "n_records", "record_bytes", "reserved0", "n_entity", "n_node", "n_photon", "lens_tag")


def parse_checkpoint_header(blob):
    """The fields of a checkpoint's header as a dict (no device needed); ValueError when the blob is not a checkpoint of this format."""
    n = struct.calcsize(CHECKPOINT_HEADER)
    if len(blob) < n:
        raise ValueError(f"checkpoint: {len(blob)} bytes, the header alone has {n}")
    v = struct.unpack(CHECKPOINT_HEADER, bytes(blob[:n]))
    if v[0] != CHECKPOINT_MAGIC:
        raise ValueError("checkpoint: bad magic")
    h = {"magic": v[0], "version": v[1], "header_bytes": v[2], "cam_pos": v[3:6], "cam_up": v[6:9], "cam_forward": v[9:12],
         "sensor_diag": v[12], "focal_dist": v[13]}
    h.update(zip(_CHECKPOINT_FIELDS, v[14:]))
    h["reserved1"] = h["lens_tag"]      # the field's name before it became the lens tag
    if h["version"] != CHECKPOINT_VERSION or h["header_bytes"] != n or h["record_bytes"] != CHECKPOINT_RECORD_BYTES:
        raise ValueError(f"checkpoint: version {h['version']}, header {h['header_bytes']} bytes, records of {h['record_bytes']} bytes: not this format")
    if len(blob) != n + h["n_records"] * CHECKPOINT_RECORD_BYTES:
        raise ValueError(f"checkpoint: {len(blob)} bytes, {n + h['n_records'] * CHECKPOINT_RECORD_BYTES} expected (truncated?)")
    return h


class ProgressiveRender:
    """A progressive render session of a RayTracer (gi_progressive_*, include/gi_hip.h): the frame is refined in steps, and a frame built in steps
    has the bits of the frame `run` builds in one call.  From RayTracer.progressive(w, h, **kw) or RayTracer.resume(blob); a context manager.
    A context has one session: opening another, or uploading a scene or photons, ends this one (its next step raises GiError, code -4).
    An object whose session was replaced by a newer one of the same RayTracer is stale: it raises the same error and its close() does nothing,
    so closing an old object never ends the newer session."""

    def __init__(self, rt, width, rows):
        self.rt, self.width, self.rows = rt, width, rows
        rt._session_serial = self.serial = getattr(rt, "_session_serial", 0) + 1

    def _mine(self):
        """Raise unless the context's session is still the one this object opened."""
        if self.rt._session_serial != self.serial:
            raise GiError(f"progressive: this session was replaced by a newer one of the same RayTracer ({GI_E_STATE})")

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def _status(self):
        self._mine()
        e, n = C.c_int32(), C.c_int64()
        self.rt._check(self.rt.L.gi_progressive_status(self.rt.h, C.byref(e), C.byref(n)), "progressive_status")
        return e.value, n.value

    @property
    def sample_end(self):
        """E: every pixel has been offered samples [0, E)."""
        return self._status()[0]

    @property
    def pixels_wanting(self):
        """Pixels of this rank that would still take a sample under the session's max_samples."""
        return self._status()[1]

    @property
    def done(self):
        return self.pixels_wanting == 0

    def step(self, n, f64=True, want_spp=False, cancel=None):
        """Take up to n more samples per pixel and return the frame so far, [rows][w][3] linear (and the samples taken per pixel with want_spp).
        cancel: an optional ctypes c_int polled during the step; a cancelled step raises GiError (code -5) and the session goes on."""
        self._mine()
        out, o = _out((self.rows, self.width, 3), f64)
        spp = np.zeros((self.rows, self.width), np.int32) if want_spp else None
        self.rt._check(self.rt.L.gi_progressive_step_host(self.rt.h, int(n), *o, _p(spp, C.c_void_p),
                                                          C.addressof(cancel) if cancel is not None else None), "progressive_step")
        return (out, spp) if want_spp else out

    def frame(self, f64=True, want_spp=False):
        """The frame as it stands (step(0): no path kernel runs)."""
        return self.step(0, f64=f64, want_spp=want_spp)

    def step_device(self, n, out_ptr, f64=False, spp_ptr=None):
        """A step into device memory (raw device pointers), asynchronous on the context's stream."""
        self._mine()
        self.rt._check(self.rt.L.gi_progressive_step_device(self.rt.h, int(n), *_dev(out_ptr, f64), spp_ptr or None, None), "progressive_step")

    def save(self):
        """The session as a checkpoint blob (bytes) for RayTracer.resume on a context with the same scene and photons."""
        self._mine()
        n = C.c_int64()
        self.rt._check(self.rt.L.gi_progressive_state_bytes(self.rt.h, C.byref(n)), "progressive_state_bytes")
        buf = C.create_string_buffer(n.value)
        self.rt._check(self.rt.L.gi_progressive_save(self.rt.h, buf, n.value), "progressive_save")
        return buf.raw

    def close(self):
        """End the session and free its records; nothing when a newer session has replaced this one."""
        if self.rt._session_serial == self.serial:
            self.rt.L.gi_progressive_end(self.rt.h)


class RayTracerGroup:
    """Several devices driven from one process through the C ABI's gi_group_* entries (include/gi_hip.h): what the C++ RayTracer::run uses when
    more than one GPU is visible.  `devices` may repeat an ordinal (several contexts on one device)."""

    def __init__(self, devices):
        self.L = lib()
        h = C.c_void_p()
        dv = np.ascontiguousarray(devices, np.int32)
        rc = self.L.gi_group_create(C.byref(h), len(dv), _p(dv, _ip))
        if rc != GI_OK:
            raise GiError(f"gi_group_create failed ({rc}): no usable HIP device -- this path has no CPU fallback")
        self.h = h
        self.n = self.L.gi_group_size(h)

    def __del__(self):
        try:
            self.L.gi_group_destroy(self.h)
        except Exception:
            pass

    def _check(self, rc, what):
        if rc < 0:
            raise GiError(f"{what}: {self.L.gi_group_last_error(self.h).decode()} ({rc})")

    def setScene(self, scene, photons=None):
        d = scene.desc()
        self._check(self.L.gi_group_upload_scene(self.h, C.byref(d)), "group upload_scene")
        self.L.gi_group_clear_photons(self.h)
        if photons is not None:
            scene.build_photon_map(photons)
            pd = scene.photon_desc()
            self._check(self.L.gi_group_upload_photons(self.h, C.byref(pd)), "group upload_photons")
        return self

    def set_lens(self, radius=None, blades=None, rotation=None, lens=None):
        """gi_group_set_lens: the thin lens of every member context (RayTracer.set_lens)."""
        l = lens if lens is not None else lens_params(radius, blades, rotation)
        self._check(self.L.gi_group_set_lens(self.h, C.byref(l)), "group set_lens")
        return self

    def run(self, params, stripe_h=16, first_stripe=0, n_stripes=None, f64=True, frame=None):
        """gi_group_render_host: the stripes of the window into a whole-frame host buffer (rows outside the window keep what `frame` held)."""
        w, h = params.width, params.height
        total = (h + stripe_h - 1) // stripe_h
        n_stripes = total if n_stripes is None else n_stripes
        out = _out((h, w, 3), f64)[0] if frame is None else frame
        self._check(self.L.gi_group_render_host(self.h, C.byref(params), stripe_h, first_stripe, n_stripes, _p(out, C.c_void_p), 1 if f64 else 0, None, None), "group render_host")
        return out

    def run_device(self, params, out_ptr, stripe_h=16, f64=False):
        """gi_group_render_device: the whole frame gathered on the first context's device (raw device pointer)."""
        self._check(self.L.gi_group_render_device(self.h, C.byref(params), stripe_h, *_dev(out_ptr, f64), None), "group render_device")
