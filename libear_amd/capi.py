"""ctypes bindings of the libearhip C ABI (include/earhip.h).

Thin and explicit on purpose: every call goes through the C ABI exactly as a foreign-language
binding would, so the GPU parity tests exercise the drop-in boundary itself.  Arrays are numpy
float32, planar ``[channels][samples]``.
"""
import ctypes as C
import os

import numpy as np

from .build import lib_path

f32p = C.POINTER(C.c_float)
i64p = C.POINTER(C.c_int64)
pp_f32 = C.POINTER(f32p)

OK, INVALID_ARGUMENT, INTERNAL_ERROR, DEVICE_ERROR, NOT_IMPLEMENTED, UNKNOWN_LAYOUT, ADM_ERROR = 0, 1, 2, 3, 4, 5, 6


class EarHipError(Exception):
    def __init__(self, code, msg):
        super().__init__(msg)
        self.code = code


class InvalidArgument(EarHipError, ValueError):
    """maps to ear::invalid_argument"""


class InternalError(EarHipError, RuntimeError):
    """maps to ear::internal_error"""


class UnknownLayout(InvalidArgument):
    """maps to ear::unknown_layout"""


class AdmError(InvalidArgument):
    """maps to ear::adm_error"""


class NotImplementedInLibear(EarHipError, RuntimeError):
    """maps to ear::not_implemented: a case libear itself refuses"""


class RenderConfig(C.Structure):
    _fields_ = [("n_objects", C.c_int), ("n_out", C.c_int), ("block_size", C.c_int),
                ("n_buses", C.c_int), ("decorrelators", f32p), ("n_taps", C.c_int),
                ("delay", C.c_int), ("max_blocks", C.c_int)]


class PcmOut(C.Structure):
    """earhip_pcm_out: the output format of Renderer.process_frames_pcm"""
    _fields_ = [("format", C.c_int), ("dither", C.c_int), ("seed", C.c_uint32)]


PROCESS_FUNC =C.CFUNCTYPE(C.c_int, pp_f32, pp_f32, C.c_void_p)

_lib = None


def load():
    """Loads libearhip.so; raises if it has not been built (no fallback of any kind)."""
    global _lib
    if _lib is not None:
        return _lib
    path = lib_path()
    if not os.path.exists(path):
        raise ImportError(f"{path} not found: run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(libear_amd has no CPU fallback)")
    lib = C.CDLL(path)
    lib.earhip_last_error.restype = C.c_char_p
    lib.earhip_conv_filter_num_blocks.restype = C.c_size_t
    lib.earhip_conv_filter_num_blocks.argtypes = [C.c_void_p]
    lib.earhip_delay_get_delay.argtypes = [C.c_void_p]
    lib.earhip_vbs_get_delay.argtypes = [C.c_void_p]
    _lib = lib
    return lib


def check(rc):
    if rc == OK:
        return
    msg = load().earhip_last_error().decode()
    if rc == INVALID_ARGUMENT:
        raise InvalidArgument(rc, msg)
    if rc == UNKNOWN_LAYOUT:
        raise UnknownLayout(rc, msg)
    if rc == ADM_ERROR:
        raise AdmError(rc, msg)
    if rc == NOT_IMPLEMENTED:
        raise NotImplementedInLibear(rc, msg)
    raise InternalError(rc, msg)


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _ptr(a, t=f32p):
    return a.ctypes.data_as(t)


def _chan_ptrs(a, offset=0):
    """float*[] over the rows of a C-contiguous [channels][samples] float32 array."""
    n = a.shape[0]
    arr = (f32p * max(n, 1))()
    base = a.ctypes.data
    for c in range(n):
        arr[c] = C.cast(base + (c * a.shape[1] + offset) * 4, f32p)
    return arr


def device_count():
    n = C.c_int(0)
    check(load().earhip_device_count(C.byref(n)))
    return n.value


class Context:
    def __init__(self, device=0, stream=None):
        self.h = C.c_void_p()
        check(load().earhip_ctx_create(device, C.c_void_p(stream) if stream else None, C.byref(self.h)))

    def set_strict(self, strict):
        check(load().earhip_ctx_set_strict(self.h, int(bool(strict))))

    def synchronize(self):
        check(load().earhip_ctx_synchronize(self.h))

    def set_option(self, key, value=None):
        """a tuning knob of this context (include/earhip.h: earhip_ctx_set_option); value None: back to the default"""
        check(load().earhip_ctx_set_option(self.h, key.encode(), None if value is None else str(value).encode()))

    def get_option(self, key):
        """None when the option is at its default, else its integer value"""
        is_set, v = C.c_int(0), C.c_int(0)
        check(load().earhip_ctx_get_option(self.h, key.encode(), C.byref(is_set), C.byref(v)))
        return v.value if is_set.value else None

    def read_bandwidth(self, dev_ptr, rows, stride, nsamples, reps=5):
        """(ms linear stream over rows*stride floats, ms gain-stage row pattern over rows*nsamples floats)"""
        ms = (C.c_double * 2)()
        check(load().earhip_debug_read_bandwidth(self.h, C.c_void_p(dev_ptr), C.c_size_t(rows), C.c_size_t(stride),
                                                 C.c_size_t(nsamples), int(reps), ms))
        return ms[0], ms[1]

    def copy_bandwidth(self, host_array, reps=3):
        """(ms host -> device, ms device -> host) of a plain copy of the array's bytes (it is overwritten with its own
        contents by the second direction)"""
        ms = (C.c_double * 2)()
        check(load().earhip_debug_copy_bandwidth(self.h, C.c_void_p(host_array.ctypes.data), C.c_size_t(host_array.nbytes), int(reps), ms))
        return ms[0], ms[1]

    # --- host memory the device reaches directly (earhip_host_alloc / _register / _release)
    def pinned_array(self, shape, dtype=np.float32):
        """array (float32 unless dtype says otherwise: int16 / int32 / uint8 for PCM frames) in pinned, device-reachable host
        memory (C-contiguous: the rows of a [channels][samples] array are evenly spaced channel buffers).  Valid until close() or
        release(array)."""
        shape = tuple(int(v) for v in np.atleast_1d(shape))
        dtype = np.dtype(dtype)
        count = int(np.prod(shape))
        p = C.c_void_p()
        nbytes = dtype.itemsize * max(count, 1)
        check(load().earhip_host_alloc(self.h, C.c_size_t(nbytes), C.byref(p)))
        buf = (C.c_char * nbytes).from_address(p.value)
        a = np.frombuffer(buf, dtype=dtype, count=count).reshape(shape)
        a[...] = 0
        return a

    def register(self, a):
        """make the memory of a C-contiguous float32 array reachable by the device (hipHostRegister)"""
        assert a.dtype == np.float32 and a.flags["C_CONTIGUOUS"]
        check(load().earhip_host_register(self.h, C.c_void_p(a.ctypes.data), C.c_size_t(a.nbytes)))

    def release(self, a):
        check(load().earhip_host_release(self.h, C.c_void_p(a.ctypes.data)))

    def close(self):
        if self.h:
            load().earhip_ctx_destroy(self.h)
            self.h = C.c_void_p()

    # --- (A) interpolation policies -------------------------------------------------
    def apply_interp(self, x, out, range_start, range_end, block_start, start, end, start_point, end_point):
        """x [n_in][n], out [n_out][n] (written in place on [range_start, range_end))."""
        sp, ep = _f32(start_point), _f32(end_point)
        n_in, n_out = x.shape[0], out.shape[0]
        assert sp.size == n_in * n_out and ep.size == n_in * n_out
        check(load().earhip_interp_apply_interp(
            self.h, n_in, n_out, _chan_ptrs(x), _chan_ptrs(out), C.c_int64(range_start), C.c_int64(range_end),
            C.c_int64(block_start), C.c_int64(start), C.c_int64(end), _ptr(sp), _ptr(ep)))

    def apply_constant(self, x, out, range_start, range_end, point):
        pt = _f32(point)
        n_in, n_out = x.shape[0], out.shape[0]
        assert pt.size == n_in * n_out
        check(load().earhip_interp_apply_constant(
            self.h, n_in, n_out, _chan_ptrs(x), _chan_ptrs(out), C.c_int64(range_start), C.c_int64(range_end),
            _ptr(pt)))


class GainInterp:
    """(A') whole-curve GainInterpolator with device-resident points."""

    def __init__(self, ctx, n_in, n_out):
        self.ctx, self.n_in, self.n_out = ctx, n_in, n_out
        self.h = C.c_void_p()
        check(load().earhip_gain_interp_create(ctx.h, n_in, n_out, C.byref(self.h)))

    def set_points(self, times, values):
        t = np.ascontiguousarray(times, dtype=np.int64)
        v = _f32(values).reshape(len(t), self.n_in, self.n_out) if len(t) else _f32(values)
        check(load().earhip_gain_interp_set_points(self.h, len(t), _ptr(t, i64p), _ptr(v)))

    def process(self, block_start, x):
        x = _f32(x).reshape(self.n_in, -1)
        out = np.zeros((self.n_out, x.shape[1]), np.float32)
        check(load().earhip_gain_interp_process(self.h, C.c_int64(block_start), C.c_size_t(x.shape[1]),
                                                _chan_ptrs(x), _chan_ptrs(out)))
        return out

    def process_device(self, block_start, nsamples, in_ptr, in_stride, out_ptr, out_stride):
        """device-resident planar buffers (16-byte aligned, strides multiples of 4); enqueues, does not synchronise"""
        check(load().earhip_gain_interp_process_device(self.h, C.c_int64(block_start), C.c_size_t(nsamples),
                                                       C.c_void_p(in_ptr), C.c_size_t(in_stride), C.c_void_p(out_ptr),
                                                       C.c_size_t(out_stride)))

    def close(self):
        if self.h:
            load().earhip_gain_interp_destroy(self.h)
            self.h = C.c_void_p()


class FFTPlan:
    def __init__(self, ctx, n_fft):
        self.n = n_fft
        self.h = C.c_void_p()
        check(load().earhip_fft_plan_create(ctx.h, C.c_size_t(n_fft), C.byref(self.h)))

    def forward(self, x):
        x = _f32(x)
        assert x.size == self.n
        out = np.empty(self.n // 2 + 1, np.complex64)
        check(load().earhip_fft_forward(self.h, _ptr(x), _ptr(out)))
        return out

    def reverse(self, X):
        X = np.ascontiguousarray(X, dtype=np.complex64)
        assert X.size == self.n // 2 + 1
        out = np.empty(self.n, np.float32)
        check(load().earhip_fft_reverse(self.h, _ptr(X), _ptr(out)))
        return out

    def close(self):
        if self.h:
            load().earhip_fft_plan_destroy(self.h)
            self.h = C.c_void_p()


class ConvCtx:
    def __init__(self, ctx, block_size):
        self.block_size = block_size
        self.h = C.c_void_p()
        check(load().earhip_conv_ctx_create(ctx.h, C.c_size_t(block_size), C.byref(self.h)))

    def close(self):
        if self.h:
            check(load().earhip_conv_ctx_destroy(self.h))
            self.h = C.c_void_p()


class ConvFilter:
    def __init__(self, cctx, taps):
        taps = _f32(taps)
        self.h = C.c_void_p()
        check(load().earhip_conv_filter_create(cctx.h, C.c_size_t(taps.size), _ptr(taps), C.byref(self.h)))

    def num_blocks(self):
        return load().earhip_conv_filter_num_blocks(self.h)

    def close(self):
        if self.h:
            check(load().earhip_conv_filter_destroy(self.h))
            self.h = C.c_void_p()


class BlockConvolver:
    def __init__(self, cctx, filt=None, num_blocks=0):
        self.B = cctx.block_size
        self.h = C.c_void_p()
        check(load().earhip_conv_create(cctx.h, filt.h if filt else None, C.c_size_t(num_blocks),
                                        C.byref(self.h)))

    def set_filter(self, f):
        check(load().earhip_conv_set_filter(self.h, f.h if f else None))

    def crossfade_filter(self, f):
        check(load().earhip_conv_crossfade_filter(self.h, f.h if f else None))

    def fade_down(self):
        self.crossfade_filter(None)

    def unset_filter(self):
        self.set_filter(None)

    def process(self, x):
        out = np.empty(self.B, np.float32)
        if x is None:
            check(load().earhip_conv_process(self.h, None, _ptr(out)))
        else:
            x = _f32(x)
            assert x.size == self.B
            check(load().earhip_conv_process(self.h, _ptr(x), _ptr(out)))
        return out

    def close(self):
        if self.h:
            check(load().earhip_conv_destroy(self.h))
            self.h = C.c_void_p()


class DelayBuffer:
    def __init__(self, ctx, nch, delay):
        self.nch = nch
        self.h = C.c_void_p()
        check(load().earhip_delay_create(ctx.h, C.c_size_t(nch), C.c_size_t(delay), C.byref(self.h)))

    def get_delay(self):
        return load().earhip_delay_get_delay(self.h)

    def process(self, x):
        x = _f32(x).reshape(self.nch, -1)
        out = np.empty_like(x)
        check(load().earhip_delay_process(self.h, C.c_size_t(x.shape[1]), _chan_ptrs(x), _chan_ptrs(out)))
        return out

    def close(self):
        if self.h:
            check(load().earhip_delay_destroy(self.h))
            self.h = C.c_void_p()


class VariableBlockSizeAdapter:
    """Host-side adapter; fn(in [n_in][B]) -> out [n_out][B]."""

    def __init__(self, block_size, n_in, n_out, fn, ctx=None, raw=False):
        """ctx: keep the FIFO buffers in device-reachable host memory of that context (earhip_vbs_create_pinned);
        raw: fn(in_ptrs, out_ptrs) gets the adapter's own channel pointer arrays (to hand on to a C entry point)"""
        self.B, self.n_in, self.n_out = block_size, n_in, n_out
        self.error = None

        def cb(inp, outp, _user):
            try:
                if raw:
                    fn(inp, outp)
                    return OK
                x = np.stack([np.ctypeslib.as_array(inp[c], (block_size,)) for c in range(n_in)])
                y = _f32(fn(x))
                for c in range(n_out):
                    np.ctypeslib.as_array(outp[c], (block_size,))[:] = y[c]
                return OK
            except Exception as e:  # surfaced by process()
                self.error = e
                return INTERNAL_ERROR

        self._cb = PROCESS_FUNC(cb)
        self.h = C.c_void_p()
        if ctx is not None:
            check(load().earhip_vbs_create_pinned(ctx.h, C.c_size_t(block_size), C.c_size_t(n_in), C.c_size_t(n_out),
                                                  self._cb, None, C.byref(self.h)))
        else:
            check(load().earhip_vbs_create(C.c_size_t(block_size), C.c_size_t(n_in), C.c_size_t(n_out), self._cb,
                                           None, C.byref(self.h)))

    def close(self):
        if self.h:
            load().earhip_vbs_destroy(self.h)
            self.h = C.c_void_p()

    def get_delay(self):
        return load().earhip_vbs_get_delay(self.h)

    def process(self, x):
        x = _f32(x).reshape(self.n_in, -1)
        n = x.shape[1]
        out = np.empty((self.n_out, n), np.float32)
        xs = x if n else np.zeros((self.n_in, 1), np.float32)
        os_ = out if n else np.zeros((self.n_out, 1), np.float32)
        rc = load().earhip_vbs_process(self.h, C.c_size_t(n), _chan_ptrs(xs), _chan_ptrs(os_))
        if self.error is not None:
            e, self.error = self.error, None
            raise e
        check(rc)
        return out


def design_decorrelators(names):
    """(G) 512-tap decorrelator FIR per channel, [n][512] float32."""
    arr = (C.c_char_p * len(names))(*[n.encode() for n in names])
    out = np.empty((len(names), load().earhip_decorrelator_size()), np.float32)
    check(load().earhip_design_decorrelators(len(names), arr, _ptr(out)))
    return out


def layout_names():
    """(H) names of the BS.2051 layouts the library knows (defined layouts are not listed: layout_kind)"""
    lib = load()
    lib.earhip_layout_name.restype = C.c_char_p
    return [lib.earhip_layout_name(i).decode() for i in range(lib.earhip_layout_count())]


def layout_channels(layout):
    """(H) [(name, azimuth, elevation, is_lfe)] of a layout (BS.2051 or defined), in layout order"""
    n = C.c_int(0)
    check(load().earhip_layout_num_channels(layout.encode(), C.byref(n)))
    out = []
    for i in range(n.value):
        name, az, el, lfe = C.c_char_p(), C.c_double(), C.c_double(), C.c_int()
        check(load().earhip_layout_channel(layout.encode(), i, C.byref(name), C.byref(az), C.byref(el), C.byref(lfe)))
        out.append((name.value.decode(), az.value, el.value, bool(lfe.value)))
    return out


def layout_channel_ranges(layout):
    """(H) [((az_lo, az_hi), (el_lo, el_hi))] per channel: where BS.2051 allows the real loudspeaker to stand"""
    n = C.c_int(0)
    check(load().earhip_layout_num_channels(layout.encode(), C.byref(n)))
    out = []
    for i in range(n.value):
        az, el = (C.c_double * 2)(), (C.c_double * 2)()
        check(load().earhip_layout_channel_ranges(layout.encode(), i, az, el))
        out.append(((az[0], az[1]), (el[0], el[1])))
    return out


class LayoutChannelDef(C.Structure):
    """earhip_layout_channel_def"""
    _fields_ = [("name", C.c_char_p), ("azimuth", C.c_double), ("elevation", C.c_double), ("has_ranges", C.c_int),
                ("azimuth_range", C.c_double * 2), ("elevation_range", C.c_double * 2), ("is_lfe", C.c_int)]


def define_layout(name, channels):
    """(H) defines a loudspeaker layout of the caller's own under `name`; every function that takes a layout name then
    accepts it.  channels: a list, in layout order, of (name, azimuth, elevation[, is_lfe[, azimuth_range,
    elevation_range]]) with the NOMINAL position in degrees and the ranges as (lo, hi) pairs (absent: the nominal
    position itself).  Pure host: the hull and a dry run of the panner's regions run here, so a bad layout raises here.
    Defining a name again with the same content does nothing; with other content it is an InvalidArgument."""
    defs = (LayoutChannelDef * max(len(channels), 1))()
    for d, ch in zip(defs, channels):
        d.name, d.azimuth, d.elevation = ch[0].encode(), float(ch[1]), float(ch[2])
        d.is_lfe = int(bool(ch[3])) if len(ch) > 3 else 0
        if len(ch) > 4:
            d.has_ranges = 1
            d.azimuth_range[0], d.azimuth_range[1] = (float(v) for v in ch[4])
            d.elevation_range[0], d.elevation_range[1] = (float(v) for v in ch[5])
    check(load().earhip_layout_define(name.encode(), len(channels), defs))


def layout_kind(name):
    """(H) 0: unknown, 1: an ITU-R BS.2051 layout, 2: a defined layout"""
    kind = C.c_int(0)
    check(load().earhip_layout_kind(name.encode(), C.byref(kind)))
    return kind.value


def layout_hull(name):
    """(H) the triangulation of a layout -> (xyz float64 [V][3], mix_to int32 [V], n_virtual, facets): the augmented
    vertices at their nominal positions, the channel of the full layout each one's gain goes to (-1: the virtual
    loudspeakers, which come last), and the hull's facets as ascending tuples of vertex indices"""
    i32 = C.POINTER(C.c_int)
    nv, nvirt, nints = C.c_int(0), C.c_int(0), C.c_int(0)
    check(load().earhip_layout_hull(name.encode(), 0, None, None, C.byref(nv), C.byref(nvirt), 0, None, C.byref(nints)))
    xyz = np.empty((nv.value, 3), np.float64)
    mix_to = np.empty(nv.value, np.int32)
    ints = np.empty(nints.value, np.int32)
    check(load().earhip_layout_hull(name.encode(), nv.value, _ptr(xyz, C.POINTER(C.c_double)), _ptr(mix_to, i32), C.byref(nv),
                                    C.byref(nvirt), nints.value, _ptr(ints, i32), C.byref(nints)))
    facets, at = [], 0
    while ints[at]:
        facets.append(tuple(int(v) for v in ints[at + 1:at + 1 + ints[at]]))
        at += 1 + int(ints[at])
    return xyz, mix_to, nvirt.value, facets


class PannerReport(C.Structure):
    """earhip_panner_report"""
    _fields_ = [("n_directions", C.c_int), ("missed", C.c_uint), ("max_power_error", C.c_double),
                ("min_own_gain", C.c_double), ("n_regions", C.c_int), ("n_triplets", C.c_int), ("n_quads", C.c_int),
                ("n_ngons", C.c_int), ("largest_ngon", C.c_int)]


def design_decorrelators_for_layout(layout, without_lfe=False):
    chans = [c for c in layout_channels(layout) if not (without_lfe and c[3])]
    out = np.empty((len(chans), load().earhip_decorrelator_size()), np.float32)
    check(load().earhip_design_decorrelators_for_layout(layout.encode(), int(without_lfe), _ptr(out)))
    return out


def design_decorrelator_basic(dec_id, size=512):
    out = np.empty(size, np.float64)
    check(load().earhip_design_decorrelator_basic(dec_id, size, _ptr(out, C.POINTER(C.c_double))))
    return out


def compensation_delay():
    return load().earhip_decorrelator_compensation_delay()


class Panner:
    """(I) gain-vector producer for Objects content (point-source pan, LFE mask, diffuse split), batched."""

    def __init__(self, ctx, layout, positions=None):
        """positions: (azimuths, elevations) in degrees of every channel of the full layout (LFE included): the
        loudspeakers' real positions; None: nominal"""
        self.h = C.c_void_p()
        if positions is None:
            check(load().earhip_panner_create(ctx.h, layout.encode(), C.byref(self.h)))
        else:
            f64 = C.POINTER(C.c_double)
            az, el = (np.ascontiguousarray(v, np.float64) for v in positions)
            assert az.size == el.size
            check(load().earhip_panner_create_positions(ctx.h, layout.encode(), int(az.size), _ptr(az, f64), _ptr(el, f64),
                                                        C.byref(self.h)))
        n = C.c_int(0)
        check(load().earhip_panner_num_channels(self.h, C.byref(n)))
        self.n_out = n.value

    def calculate(self, az, el, dist=None, gain=None, diffuse=None, width=None, height=None, depth=None):
        """arrays [n] (degrees) -> (direct, diffuse) float32 [n][n_out]; width / height / depth: the extent
        panner (all None: point sources)"""
        f64 = C.POINTER(C.c_double)
        az = np.ascontiguousarray(np.atleast_1d(az), np.float64)
        n = az.size

        def arr(v):
            return None if v is None else np.ascontiguousarray(np.broadcast_to(np.asarray(v, np.float64), (n,)))

        def opt(v):
            return None if v is None else _ptr(v, f64)
        el, dist, gain, diffuse = arr(el), arr(dist), arr(gain), arr(diffuse)
        width, height, depth = arr(width), arr(height), arr(depth)
        d = np.empty((n, self.n_out), np.float32)
        f = np.empty((n, self.n_out), np.float32)
        if width is None and height is None and depth is None:
            check(load().earhip_panner_calculate(self.h, C.c_size_t(n), _ptr(az, f64), _ptr(el, f64), opt(dist), opt(gain),
                                                 opt(diffuse), _ptr(d), _ptr(f)))
        else:
            check(load().earhip_panner_calculate_extent(self.h, C.c_size_t(n), _ptr(az, f64), _ptr(el, f64), opt(dist),
                                                        opt(width), opt(height), opt(depth), opt(gain), opt(diffuse),
                                                        _ptr(d), _ptr(f)))
        return d, f

    def calculate_device(self, n, az, el, dist, gain, diffuse, direct, diffuse_out, width=None, height=None, depth=None):
        """device addresses (ints; None = absent): enqueues on the context's stream, does not synchronise"""
        def vp(a):
            return None if a is None else C.c_void_p(int(a))
        check(load().earhip_panner_calculate_extent_device(self.h, C.c_size_t(n), vp(az), vp(el), vp(dist), vp(width), vp(height),
                                                           vp(depth), vp(gain), vp(diffuse), vp(direct), vp(diffuse_out)))

    def calculate_objects(self, az, el, dist=None, gain=None, diffuse=None, width=None, height=None, depth=None,
                          channel_lock=None, lock_max_distance=None, divergence=None, azimuth_range=None, excluded=None):
        """calculate() plus channelLock (flags, and maxDistance: inf = none), polar objectDivergence (value in [0, 1],
        azimuthRange in degrees, None: 45) and zoneExclusion (bit masks over the full layout, see
        objects_excluded_channels); arrays [n] or scalars, None = absent -> (direct, diffuse) float32 [n][n_out]"""
        f64 = C.POINTER(C.c_double)
        az = np.ascontiguousarray(np.atleast_1d(az), np.float64)
        n = az.size

        def arr(v, dtype=np.float64):
            return None if v is None else np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype), (n,)))

        def opt(v, t=f64):
            return None if v is None else _ptr(v, t)
        a = [arr(v) for v in (el, dist, width, height, depth, gain, diffuse)]
        lock, mask = arr(channel_lock, np.uint8), arr(excluded, np.uint32)
        lock_max, div, rng = arr(lock_max_distance), arr(divergence), arr(azimuth_range)
        d = np.empty((n, self.n_out), np.float32)
        f = np.empty((n, self.n_out), np.float32)
        check(load().earhip_panner_calculate_objects(self.h, C.c_size_t(n), _ptr(az, f64), *[opt(v) for v in a],
                                                     opt(lock, C.POINTER(C.c_ubyte)), opt(lock_max), opt(div), opt(rng),
                                                     opt(mask, C.POINTER(C.c_uint32)), _ptr(d), _ptr(f)))
        return d, f

    def calculate_objects_device(self, n, az, el, dist, gain, diffuse, direct, diffuse_out, width=None, height=None, depth=None,
                                 channel_lock=None, lock_max_distance=None, divergence=None, azimuth_range=None, excluded=None):
        """device addresses (ints; None = absent; channel_lock: uint8, excluded: uint32, the others float64): enqueues on
        the context's stream, does not synchronise.  The values are not validated: see include/earhip.h."""
        def vp(a):
            return None if a is None else C.c_void_p(int(a))
        check(load().earhip_panner_calculate_objects_device(
            self.h, C.c_size_t(n), vp(az), vp(el), vp(dist), vp(width), vp(height), vp(depth), vp(gain), vp(diffuse),
            vp(channel_lock), vp(lock_max_distance), vp(divergence), vp(azimuth_range), vp(excluded), vp(direct), vp(diffuse_out)))

    def missed(self):
        """positions of the last calculate_device call that no region of the layout took (synchronises)"""
        n = C.c_uint(0)
        check(load().earhip_panner_missed(self.h, C.byref(n)))
        return n.value

    def self_check(self):
        """pans the 5200 directions of the HOA design's t-design and every loudspeaker's real direction in one launch
        (synchronises) -> a PannerReport: missed, max_power_error, min_own_gain and the region counts"""
        report = PannerReport()
        check(load().earhip_panner_self_check(self.h, C.byref(report)))
        return report

    def close(self):
        if self.h:
            load().earhip_panner_destroy(self.h)
            self.h = C.c_void_p()


class ExclusionZone(C.Structure):
    """earhip_exclusion_zone"""
    _fields_ = [("cartesian", C.c_int)] + [(k, C.c_double) for k in (
        "min_azimuth", "max_azimuth", "min_elevation", "max_elevation", "min_x", "max_x", "min_y", "max_y", "min_z", "max_z")]


def objects_lock_priority(layout):
    """(I) full-layout indices of a layout's non-LFE loudspeakers in channel-lock priority order (pure host)"""
    n = sum(1 for c in layout_channels(layout) if not c[3])
    order = (C.c_int * n)()
    check(load().earhip_objects_lock_priority(layout.encode(), order))
    return list(order)


def _zones(zones):
    """a list of dicts of keyword bounds -> ExclusionZone[]; a zone with any of min_x .. max_z is a Cartesian one"""
    zs = (ExclusionZone * max(len(zones), 1))()
    for z, given in zip(zs, zones):
        z.cartesian = int(any(k.endswith(("_x", "_y", "_z")) for k in given))
        for k, v in given.items():
            setattr(z, k, float(v))
    return zs


def objects_excluded_channels(layout, zones):
    """(I) the bit mask (full layout) of the loudspeakers a list of zones excludes (pure host).  A zone is a dict of
    keyword bounds: min_azimuth, max_azimuth, min_elevation, max_elevation, or min_x .. max_z (a Cartesian zone)"""
    mask = C.c_uint32(0)
    check(load().earhip_objects_excluded_channels(layout.encode(), len(zones), _zones(zones), C.byref(mask)))
    return mask.value


def objects_zone_downmix(layout, mask):
    """(I) the zone-exclusion downmix matrix [n][n] float64 of an excluded set (bit mask over the full layout; pure host)"""
    n = len(layout_channels(layout))
    out = np.empty((n, n), np.float64)
    check(load().earhip_objects_zone_downmix(layout.encode(), C.c_uint32(int(mask)), _ptr(out, C.POINTER(C.c_double))))
    return out


class DSMetadata(C.Structure):
    """earhip_ds_metadata: one DirectSpeakers channel's metadata"""
    _fields_ = [("n_labels", C.c_int), ("labels", C.POINTER(C.c_char_p)), ("cartesian", C.c_int),
                ("azimuth", C.c_double), ("elevation", C.c_double), ("distance", C.c_double)]
    _fields_ += [("has_" + k, C.c_int) for k in ("azimuth_min", "azimuth_max", "elevation_min", "elevation_max",
                                                 "distance_min", "distance_max")]
    _fields_ += [(k, C.c_double) for k in ("azimuth_min", "azimuth_max", "elevation_min", "elevation_max",
                                           "distance_min", "distance_max")]
    _fields_ += [("screen_edge_lock_horizontal", C.c_int), ("screen_edge_lock_vertical", C.c_int),
                 ("has_low_pass", C.c_int), ("has_high_pass", C.c_int), ("low_pass", C.c_double),
                 ("high_pass", C.c_double), ("audio_pack_format_id", C.c_char_p)]


class DSCartesian(C.Structure):
    """earhip_ds_cartesian: the Cartesian position of one DirectSpeakers channel (group X)"""
    _fields_ = [("x", C.c_double), ("y", C.c_double), ("z", C.c_double)]
    _fields_ += [("has_" + k, C.c_int) for k in ("x_min", "x_max", "y_min", "y_max", "z_min", "z_max")]
    _fields_ += [(k, C.c_double) for k in ("x_min", "x_max", "y_min", "y_max", "z_min", "z_max")]


BOUNDS = ("azimuth_min", "azimuth_max", "elevation_min", "elevation_max", "distance_min", "distance_max")

# Warning::Code values (libear_amd/host/ear/warnings.hpp)
FREQ_SPEAKERLABEL_LFE_MISMATCH, FREQ_NOT_LFE = 1, 2


class DirectSpeakers:
    """(I, DirectSpeakers) gain vectors for channel-based content (ear::GainCalculatorDirectSpeakers), batched.

    A channel's metadata is a dict with the keys of libear's DirectSpeakersTypeMetadata, all optional:
    speakerLabels (list of str), azimuth / elevation / distance (polar position, default 0, 0, 1), azimuthMin ...
    distanceMax (bounds), cartesian, screenEdgeLock ({"horizontal": ..., "vertical": ...}), lowPass / highPass
    (channelFrequency), audioPackFormatID."""

    _KEYS = {"azimuthMin": "azimuth_min", "azimuthMax": "azimuth_max", "elevationMin": "elevation_min",
             "elevationMax": "elevation_max", "distanceMin": "distance_min", "distanceMax": "distance_max"}

    def __init__(self, ctx, layout, substitutions=None, positions=None):
        """ctx: a Context, or None (no device panner: a non-LFE channel that needs it is an InvalidArgument);
        substitutions: {label: nominal label} on top of libear's defaults; positions: (azimuths, elevations) of
        every channel of the full layout (the loudspeakers' real positions), None: nominal"""
        subst = list((substitutions or {}).items())
        frm = (C.c_char_p * max(len(subst), 1))(*[k.encode() for k, _ in subst])
        to = (C.c_char_p * max(len(subst), 1))(*[v.encode() for _, v in subst])
        self.h = C.c_void_p()
        h = ctx.h if ctx is not None else None
        if positions is None:
            check(load().earhip_direct_speakers_create(h, layout.encode(), len(subst), frm, to, C.byref(self.h)))
        else:
            f64 = C.POINTER(C.c_double)
            az, el = (np.ascontiguousarray(v, np.float64) for v in positions)
            assert az.size == el.size
            check(load().earhip_direct_speakers_create_positions(h, layout.encode(), int(az.size), _ptr(az, f64),
                                                                 _ptr(el, f64), len(subst), frm, to, C.byref(self.h)))
        n = C.c_int(0)
        check(load().earhip_direct_speakers_num_channels(self.h, C.byref(n)))
        self.n_out = n.value

    @classmethod
    def _struct(cls, m, keep):
        s = DSMetadata()
        labels = [lab.encode() for lab in m.get("speakerLabels", ())]
        arr = (C.c_char_p * max(len(labels), 1))(*labels)
        keep.append(arr)
        s.n_labels, s.labels = len(labels), C.cast(arr, C.POINTER(C.c_char_p))
        s.cartesian = int(bool(m.get("cartesian", False)))
        s.azimuth, s.elevation, s.distance = m.get("azimuth", 0.0), m.get("elevation", 0.0), m.get("distance", 1.0)
        for k, f in cls._KEYS.items():
            if m.get(k) is not None:
                setattr(s, "has_" + f, 1)
                setattr(s, f, m[k])
        sel = m.get("screenEdgeLock") or {}
        s.screen_edge_lock_horizontal = int(sel.get("horizontal") is not None)
        s.screen_edge_lock_vertical = int(sel.get("vertical") is not None)
        if m.get("lowPass") is not None:
            s.has_low_pass, s.low_pass = 1, m["lowPass"]
        if m.get("highPass") is not None:
            s.has_high_pass, s.high_pass = 1, m["highPass"]
        pack = m.get("audioPackFormatID")
        s.audio_pack_format_id = None if pack is None else pack.encode()
        return s

    def calculate(self, metadata):
        """list of metadata dicts [n] -> (gains float32 [n][n_out], warnings int32 [n][2]: Warning::Code values in
        the order libear raises them, 0 where none)"""
        n = len(metadata)
        keep = []
        md = (DSMetadata * max(n, 1))(*[self._struct(m, keep) for m in metadata])
        gains = np.zeros((n, self.n_out), np.float32)
        warnings = np.zeros((n, 2), np.int32)
        self.last_warnings = warnings
        check(load().earhip_direct_speakers_calculate(self.h, C.c_size_t(n), md, _ptr(gains),
                                                      _ptr(warnings, C.POINTER(C.c_int))))
        return gains, warnings

    _CART_KEYS = {"XMin": "x_min", "XMax": "x_max", "YMin": "y_min", "YMax": "y_max", "ZMin": "z_min", "ZMax": "z_max"}
    _LOCK_CODES = ({None: 0, "left": 1, "right": 2}, {None: 0, "bottom": 1, "top": 2})

    def calculate_screen(self, metadata, reproduction=None):
        """(X) calculate for beds with Cartesian positions and screenEdgeLock.  The same dicts, plus X, Y, Z (the presence of
        X makes the position Cartesian; Y defaults to 1, Z to 0) with XMin ... ZMax; screenEdgeLock {"horizontal": "left" |
        "right", "vertical": "bottom" | "top"} (or group R's codes 0, 1, 2) locks the position to an edge of `reproduction`
        (a Screen; None: no screen, a lock changes nothing).  -> (gains, warnings) as calculate"""
        n = len(metadata)
        keep = []
        md = (DSMetadata * max(n, 1))()
        cart = (DSCartesian * max(n, 1))()
        for i, m in enumerate(metadata):
            md[i] = self._struct(m, keep)
            sel = m.get("screenEdgeLock") or {}
            for field, key, codes in zip(("screen_edge_lock_horizontal", "screen_edge_lock_vertical"),
                                         ("horizontal", "vertical"), self._LOCK_CODES):
                v = sel.get(key)
                if isinstance(v, (int, np.integer)):
                    code = int(v)
                elif v in codes:
                    code = codes[v]
                else:
                    raise InvalidArgument(1, f"metadata[{i}]: invalid {key} screenEdgeLock: {v!r}")
                setattr(md[i], field, code)
            if m.get("X") is not None or m.get("cartesian"):
                md[i].cartesian = 1
                cart[i].x, cart[i].y, cart[i].z = m.get("X", 0.0), m.get("Y", 1.0), m.get("Z", 0.0)
                for k, f in self._CART_KEYS.items():
                    if m.get(k) is not None:
                        setattr(cart[i], "has_" + f, 1)
                        setattr(cart[i], f, m[k])
        gains = np.zeros((n, self.n_out), np.float32)
        warnings = np.zeros((n, 2), np.int32)
        self.last_warnings = warnings
        check(load().earhip_direct_speakers_calculate_screen(self.h, _screen_ref(reproduction), C.c_size_t(n), md, cart,
                                                             _ptr(gains), _ptr(warnings, C.POINTER(C.c_int))))
        return gains, warnings

    def cartesian_positions(self):
        """(X) -> (nominal, real) float64 [n_out][3]: the loudspeakers as the Cartesian bounds test and the nearest-candidate
        rule see them, group K's point conversion of the nominal and of the real positions at distance 1"""
        f64 = C.POINTER(C.c_double)
        nominal, real = np.empty((self.n_out, 3), np.float64), np.empty((self.n_out, 3), np.float64)
        check(load().earhip_direct_speakers_cartesian_positions(self.h, _ptr(nominal, f64), _ptr(real, f64)))
        return nominal, real

    def missed(self):
        """channels of the last calculate that no region of the point source panner took"""
        n = C.c_uint(0)
        check(load().earhip_direct_speakers_missed(self.h, C.byref(n)))
        return n.value

    def close(self):
        if self.h:
            load().earhip_direct_speakers_destroy(self.h)
            self.h = C.c_void_p()


# (K) conversion of Objects metadata between polar and Cartesian (ear::conversion)

def _conv_host(fn, pos, extent):
    f64 = C.POINTER(C.c_double)
    pos = [np.ascontiguousarray(np.atleast_1d(v), np.float64) for v in pos]
    n = pos[0].size
    assert all(v.size == n for v in pos), "the position arrays must have one size"
    ext_in = [None if v is None else np.ascontiguousarray(np.broadcast_to(np.asarray(v, np.float64), (n,)))
              for v in (extent if extent is not None else (None, None, None))]
    out = [np.empty(n, np.float64) for _ in range(3)]
    ext_out = [np.empty(n, np.float64) for _ in range(3)] if extent is not None else [None] * 3

    def opt(v):
        return None if v is None else _ptr(v, f64)
    check(fn(C.c_size_t(n), *[_ptr(v, f64) for v in pos], *[opt(v) for v in ext_in], *[_ptr(v, f64) for v in out],
             *[opt(v) for v in ext_out]))
    return tuple(out) if extent is None else (tuple(out), tuple(ext_out))


def to_polar(x, y, z, width=None, height=None, depth=None, extent=None):
    """Cartesian -> polar on the calling thread (libear's pointCartToPolar / extentCartToPolar; no device needed).
    Arrays [n] -> (azimuth, elevation, distance); with extents (extent=True, or any of width / height / depth given;
    a missing one is 0) -> ((azimuth, elevation, distance), (width, height, depth)).  Raises on the first failing
    element, the message naming its index."""
    if extent is None:
        extent = width is not None or height is not None or depth is not None
    return _conv_host(load().earhip_conversion_to_polar, (x, y, z), (width, height, depth) if extent else None)


def to_cartesian(azimuth, elevation, distance, width=None, height=None, depth=None, extent=None):
    """polar -> Cartesian on the calling thread (pointPolarToCart / extentPolarToCart), as to_polar"""
    if extent is None:
        extent = width is not None or height is not None or depth is not None
    return _conv_host(load().earhip_conversion_to_cartesian, (azimuth, elevation, distance),
                      (width, height, depth) if extent else None)


def _dev_ptr(a, n, dtype_name):
    """a device address: an int, None (absent), or a tensor on the device with n elements of the named dtype"""
    if a is None or isinstance(a, int):
        return None if a is None else C.c_void_p(a)
    assert a.is_cuda and a.is_contiguous(), "device tensors must be contiguous and on the GPU"
    assert str(a.dtype) == "torch." + dtype_name and a.numel() >= n, (a.dtype, a.numel(), n)
    return C.c_void_p(a.data_ptr())


def _conv_device(fn, ctx, n, pos, extent, out, ext_out, status):
    ext = extent if extent is not None else (None, None, None)
    eo = ext_out if ext_out is not None else (None, None, None)
    args = [_dev_ptr(v, n, "float64") for v in (*pos, *ext, *out, *eo)]
    check(fn(ctx.h, C.c_size_t(n), *args, _dev_ptr(status, n, "int32")))


def to_polar_device(ctx, n, x, y, z, azimuth, elevation, distance, width=None, height=None, depth=None,
                    width_out=None, height_out=None, depth_out=None, status=None):
    """Cartesian -> polar on the device: float64 tensors (or device addresses) of n elements, status an int32
    tensor [n] of per-element codes (may be None).  Enqueues on the context's stream and does not synchronise.
    An output may be the input tensor of the same component (in place)."""
    ext_out = None if width_out is None and height_out is None and depth_out is None else (width_out, height_out,
                                                                                          depth_out)
    _conv_device(load().earhip_conversion_to_polar_device, ctx, n, (x, y, z), (width, height, depth),
                 (azimuth, elevation, distance), ext_out, status)


def to_cartesian_device(ctx, n, azimuth, elevation, distance, x, y, z, width=None, height=None, depth=None,
                        width_out=None, height_out=None, depth_out=None, status=None):
    """polar -> Cartesian on the device, as to_polar_device"""
    ext_out = None if width_out is None and height_out is None and depth_out is None else (width_out, height_out,
                                                                                          depth_out)
    _conv_device(load().earhip_conversion_to_cartesian_device, ctx, n, (azimuth, elevation, distance),
                 (width, height, depth), (x, y, z), ext_out, status)


class Comm:
    """(J) RCCL communicator of the multi-GPU exchange: one per rank, made from rank 0's 128-byte id"""

    @staticmethod
    def unique_id():
        buf = (C.c_char * 128)()
        check(load().earhip_comm_unique_id(buf))
        return bytes(buf)

    @staticmethod
    def channel_range(n_out, rank, world):
        pad, lo, hi = C.c_int(), C.c_int(), C.c_int()
        check(load().earhip_comm_channel_range(n_out, rank, world, C.byref(pad), C.byref(lo), C.byref(hi)))
        return pad.value, lo.value, hi.value

    def __init__(self, ctx, rank, world, uid):
        assert len(uid) == 128
        self.rank, self.world = rank, world
        self.h = C.c_void_p()
        check(load().earhip_comm_create(ctx.h, rank, world, uid, C.byref(self.h)))

    def exchange_device(self, slot, partial_ptr, owned_ptr, rows_per_rank, row_stride):
        check(load().earhip_render_exchange_device(self.h, int(slot), C.c_void_p(partial_ptr), C.c_void_p(owned_ptr),
                                                   C.c_size_t(rows_per_rank), C.c_size_t(row_stride)))

    def gather_device(self, slot, owned_ptr, full_ptr, rows_per_rank, row_stride, root=-1):
        """the owned slices of all ranks -> full [world * rows_per_rank][row_stride] on every rank (root < 0) or on
        `root` only (full_ptr may be None elsewhere)"""
        check(load().earhip_comm_gather_device(self.h, int(slot), C.c_void_p(owned_ptr),
                                               C.c_void_p(full_ptr) if full_ptr else None, C.c_size_t(rows_per_rank),
                                               C.c_size_t(row_stride), int(root)))

    def wait(self, slot):
        """orders the context's stream behind the last exchange / gather issued with this slot"""
        check(load().earhip_comm_wait(self.h, int(slot)))

    def last_exchange_ms(self, slot):
        ms = C.c_double(0.0)
        check(load().earhip_comm_last_exchange_ms(self.h, int(slot), C.byref(ms)))
        return ms.value

    def info(self):
        """what RCCL says about the communicator: ranks (ncclCommCount), this rank, its HIP device, the RCCL version"""
        v = (C.c_int * 4)()
        check(load().earhip_comm_info(self.h, v))
        return {"ranks": v[0], "rank": v[1], "device": v[2], "version": v[3]}

    def link_probe(self, nbytes=50 << 20, shift=1, reps=5):
        """GB/s a rank sends to rank + shift while it receives from rank - shift (collective; 0 with one rank)"""
        g = C.c_double(0.0)
        check(load().earhip_comm_link_probe(self.h, C.c_size_t(nbytes), int(shift), int(reps), C.byref(g)))
        return g.value

    def close(self):
        if self.h:
            load().earhip_comm_destroy(self.h)
            self.h = C.c_void_p()


def hoa_decode_matrix(ctx, layout, orders, degrees, normalization="SN3D", positions=None):
    """(I, HOA) AllRAD decode matrix [n_channels][n_coef] float32; positions: real loudspeaker positions as for Panner"""
    o = np.ascontiguousarray(orders, np.int32)
    d = np.ascontiguousarray(degrees, np.int32)
    if len(o) != len(d):
        raise InvalidArgument(INVALID_ARGUMENT, "orders and degrees must be the same size")
    n = len(layout_channels(layout))
    out = np.zeros((n, max(len(o), 1)), np.float32)
    ip = C.POINTER(C.c_int)
    if positions is None:
        check(load().earhip_hoa_decode_matrix(ctx.h, layout.encode(), len(o), o.ctypes.data_as(ip), d.ctypes.data_as(ip),
                                              normalization.encode(), _ptr(out)))
    else:
        f64 = C.POINTER(C.c_double)
        az, el = (np.ascontiguousarray(v, np.float64) for v in positions)
        check(load().earhip_hoa_decode_matrix_positions(ctx.h, layout.encode(), int(az.size), _ptr(az, f64), _ptr(el, f64),
                                                        len(o), o.ctypes.data_as(ip), d.ctypes.data_as(ip),
                                                        normalization.encode(), _ptr(out)))
    return out[:, :len(o)]


# (Q) Ambisonic encoder for Objects and the rotation of the HOA bus

def _hoa_channels(orders, degrees):
    o = np.ascontiguousarray(orders, np.int32).reshape(-1)
    d = np.ascontiguousarray(degrees, np.int32).reshape(-1)
    if len(o) != len(d):
        raise InvalidArgument(INVALID_ARGUMENT, "orders and degrees must be the same size")
    ip = C.POINTER(C.c_int)
    return len(o), o, d, o.ctypes.data_as(ip), d.ctypes.data_as(ip)


def hoa_acn(order):
    """(orders, degrees) of the (order + 1)^2 channels in ACN order (AmbiX)"""
    n = (max(int(order), 0) + 1) ** 2
    o, d = np.zeros(n, np.int32), np.zeros(n, np.int32)
    ip = C.POINTER(C.c_int)
    check(load().earhip_hoa_acn(int(order), o.ctypes.data_as(ip), d.ctypes.data_as(ip)))
    return o, d


def hoa_encode(orders, degrees, az, el, gain=None, normalization="SN3D"):
    """Objects positions (ADM polar degrees) -> the gain rows of an Ambisonics bus, float32 [n][n_coef], on the calling
    thread (no device needed).  Raises on the first element that is not finite or has |el| > 90, the message naming it."""
    f64 = C.POINTER(C.c_double)
    nc, _o, _d, op, dp = _hoa_channels(orders, degrees)
    az = np.ascontiguousarray(np.atleast_1d(az), np.float64)
    n = az.size
    el = np.ascontiguousarray(np.broadcast_to(np.asarray(el, np.float64), (n,)))
    g = None if gain is None else np.ascontiguousarray(np.broadcast_to(np.asarray(gain, np.float64), (n,)))
    out = np.zeros((n, max(nc, 1)), np.float32)
    check(load().earhip_hoa_encode(nc, op, dp, normalization.encode(), C.c_size_t(n), _ptr(az, f64), _ptr(el, f64),
                                   None if g is None else _ptr(g, f64), _ptr(out)))
    return out[:, :nc]


def hoa_encode_device(ctx, n, az, el, gain, out, orders, degrees, normalization="SN3D", status=None):
    """the same on the device: float64 tensors (or device addresses) of n elements, gain may be None (1), out a float32
    tensor [n][n_coef], status an int32 tensor [n] (may be None): 1 and a row of NaN for an element hoa_encode refuses.
    Enqueues one kernel on the context's stream and does not synchronise."""
    nc, _o, _d, op, dp = _hoa_channels(orders, degrees)
    check(load().earhip_hoa_encode_device(ctx.h, nc, op, dp, normalization.encode(), C.c_size_t(n),
                                          _dev_ptr(az, n, "float64"), _dev_ptr(el, n, "float64"),
                                          _dev_ptr(gain, n, "float64"), _dev_ptr(out, n * nc, "float32"),
                                          _dev_ptr(status, n, "int32")))


def hoa_rotation_matrix(orders, degrees, q, normalization="SN3D"):
    """float32 [n_coef][n_coef] R with encode(q u) = R encode(u); q: a proper rotation, 3 x 3, acting on ADM Cartesian
    column vectors (x right, y front, z up)"""
    nc, _o, _d, op, dp = _hoa_channels(orders, degrees)
    q = np.ascontiguousarray(q, np.float64)
    if q.size != 9:
        raise InvalidArgument(INVALID_ARGUMENT, "q must have 9 entries")
    out = np.zeros((max(nc, 1), max(nc, 1)), np.float32)
    check(load().earhip_hoa_rotation_matrix(nc, op, dp, normalization.encode(), _ptr(q, C.POINTER(C.c_double)), _ptr(out)))
    return out[:nc, :nc]


# (R) the screen of an Objects block: screenRef scaling and screenEdgeLock

class Screen(C.Structure):
    """earhip_screen: a PolarScreen (cartesian 0) or a CartesianScreen"""
    _fields_ = [("cartesian", C.c_int)] + [(k, C.c_double) for k in (
        "aspect_ratio", "azimuth", "elevation", "distance", "x", "y", "z", "width_azimuth", "width_x")]

    @classmethod
    def polar(cls, aspect_ratio, azimuth, elevation, distance, width_azimuth):
        return cls(0, aspect_ratio, azimuth, elevation, distance, 0.0, 0.0, 0.0, width_azimuth, 0.0)

    @classmethod
    def cart(cls, aspect_ratio, x, y, z, width_x):
        return cls(1, aspect_ratio, 0.0, 0.0, 0.0, x, y, z, 0.0, width_x)


def _screen_ref(s):
    return None if s is None else C.byref(s)


def screen_default():
    """the default reference screen: polar, 1.78, straight ahead at distance 1, 58 degrees wide"""
    s = Screen()
    check(load().earhip_screen_default(C.byref(s)))
    return s


def screen_edges(screen):
    """(left azimuth, right azimuth, bottom elevation, top elevation) of a screen, degrees (pure host)"""
    e = (C.c_double * 4)()
    check(load().earhip_screen_edges(C.byref(screen), e))
    return tuple(e)


def screen_apply(az, el, reproduction, reference=None, screen_ref=None, lock_horizontal=None, lock_vertical=None):
    """screenRef scaling from `reference` (None: the default screen) to `reproduction` (None: no screen, everything passes
    through), then screenEdgeLock, on the calling thread (no device needed).  Arrays [n] in degrees -> (azimuth, elevation).
    screen_ref: flags, None = all set; lock_horizontal: 0 none, 1 left, 2 right; lock_vertical: 0 none, 1 bottom, 2 top; None =
    none.  Raises on the first element it refuses, the message naming its index."""
    f64, u8 = C.POINTER(C.c_double), C.POINTER(C.c_ubyte)
    az = np.ascontiguousarray(np.atleast_1d(az), np.float64)
    n = az.size
    el = np.ascontiguousarray(np.broadcast_to(np.asarray(el, np.float64), (n,)))
    flags = [None if v is None else np.ascontiguousarray(np.broadcast_to(np.asarray(v, np.uint8), (n,)))
             for v in (screen_ref, lock_horizontal, lock_vertical)]
    az_out, el_out = np.empty(n, np.float64), np.empty(n, np.float64)
    check(load().earhip_screen_apply(_screen_ref(reference), _screen_ref(reproduction), C.c_size_t(n), _ptr(az, f64),
                                     _ptr(el, f64), *[None if v is None else _ptr(v, u8) for v in flags], _ptr(az_out, f64),
                                     _ptr(el_out, f64)))
    return az_out, el_out


def screen_apply_device(ctx, n, az, el, az_out, el_out, reproduction, reference=None, screen_ref=None, lock_horizontal=None,
                        lock_vertical=None, status=None):
    """the same on the device: float64 tensors (or device addresses) of n elements, the flags uint8 tensors, status an int32
    tensor [n] (may be None): 1 and NaN outputs for an element screen_apply refuses.  An output may be its own input (in
    place).  Enqueues one kernel on the context's stream and does not synchronise."""
    check(load().earhip_screen_apply_device(ctx.h, _screen_ref(reference), _screen_ref(reproduction), C.c_size_t(n),
                                            _dev_ptr(az, n, "float64"), _dev_ptr(el, n, "float64"),
                                            _dev_ptr(screen_ref, n, "uint8"), _dev_ptr(lock_horizontal, n, "uint8"),
                                            _dev_ptr(lock_vertical, n, "uint8"), _dev_ptr(az_out, n, "float64"),
                                            _dev_ptr(el_out, n, "float64"), _dev_ptr(status, n, "int32")))


# (V) the same stage on Cartesian positions, in front of the allocentric panner

def screen_apply_cartesian(x, y, z, reproduction, reference=None, screen_ref=None, lock_horizontal=None, lock_vertical=None):
    """screenRef scaling from `reference` (None: the default screen) to `reproduction` (None: no screen, everything passes
    through), then screenEdgeLock, of Cartesian positions, on the calling thread (no device needed): to polar, the polar
    steps of screen_apply, back to Cartesian.  Arrays [n] -> (x, y, z).  screen_ref: flags, None = all set; lock_horizontal: 0
    none, 1 left, 2 right; lock_vertical: 0 none, 1 bottom, 2 top; None = none.  An element with no flag set keeps its bits.
    Raises on the first element it refuses, the message naming its index."""
    f64, u8 = C.POINTER(C.c_double), C.POINTER(C.c_ubyte)
    x = np.ascontiguousarray(np.atleast_1d(x), np.float64)
    n = x.size
    y, z = (np.ascontiguousarray(np.broadcast_to(np.asarray(v, np.float64), (n,))) for v in (y, z))
    flags = [None if v is None else np.ascontiguousarray(np.broadcast_to(np.asarray(v, np.uint8), (n,)))
             for v in (screen_ref, lock_horizontal, lock_vertical)]
    out = [np.empty(n, np.float64) for _ in range(3)]
    check(load().earhip_screen_apply_cartesian(_screen_ref(reference), _screen_ref(reproduction), C.c_size_t(n), _ptr(x, f64),
                                               _ptr(y, f64), _ptr(z, f64), *[None if v is None else _ptr(v, u8) for v in flags],
                                               *[_ptr(v, f64) for v in out]))
    return tuple(out)


def screen_apply_cartesian_device(ctx, n, x, y, z, x_out, y_out, z_out, reproduction, reference=None, screen_ref=None,
                                  lock_horizontal=None, lock_vertical=None, status=None):
    """the same on the device: float64 tensors (or device addresses) of n elements, the flags uint8 tensors, status an int32
    tensor [n] (may be None): a non-zero code and NaN outputs for an element screen_apply_cartesian refuses.  An output may be
    its own input (in place).  Enqueues one kernel on the context's stream and does not synchronise."""
    check(load().earhip_screen_apply_cartesian_device(
        ctx.h, _screen_ref(reference), _screen_ref(reproduction), C.c_size_t(n), *[_dev_ptr(v, n, "float64") for v in (x, y, z)],
        _dev_ptr(screen_ref, n, "uint8"), _dev_ptr(lock_horizontal, n, "uint8"), _dev_ptr(lock_vertical, n, "uint8"),
        *[_dev_ptr(v, n, "float64") for v in (x_out, y_out, z_out)], _dev_ptr(status, n, "int32")))


# (T) the allocentric (Cartesian) point-source panner for Objects

class Allo:
    """earhip_allo: the loudspeakers of a layout on the cube (pure host: no context, no device).  positions: float64
    [n_channels][3] (x right, y front, z up), one row per channel of the full layout, LFE rows ignored; None: the built-in
    table of the BS.2051 layouts."""

    def __init__(self, layout, positions=None):
        self.h = C.c_void_p()
        f64 = C.POINTER(C.c_double)
        if positions is None:
            check(load().earhip_allo_create(layout.encode(), C.byref(self.h)))
        else:
            p = np.ascontiguousarray(positions, np.float64)
            if p.ndim != 2 or p.shape[1] != 3:
                raise InvalidArgument(INVALID_ARGUMENT, "positions must be [n_channels][3]")
            x, y, z = (np.ascontiguousarray(p[:, k]) for k in range(3))
            check(load().earhip_allo_create_positions(layout.encode(), len(p), _ptr(x, f64), _ptr(y, f64), _ptr(z, f64),
                                                      C.byref(self.h)))
        n = C.c_int(0)
        check(load().earhip_allo_num_channels(self.h, C.byref(n)))
        self.n_out = n.value

    def positions(self):
        """the snapped positions, float64 [n_channels][3]; the rows of LFE channels are NaN"""
        xyz = np.empty((self.n_out, 3), np.float64)
        check(load().earhip_allo_positions(self.h, _ptr(xyz, C.POINTER(C.c_double))))
        return xyz

    def excluded_channels(self, zones):
        """the bit mask (full layout) of the loudspeakers a list of Cartesian zones excludes, at the handle's positions; a
        zone is a dict of keyword bounds min_x .. max_z (a polar zone is an InvalidArgument)"""
        mask = C.c_uint32(0)
        check(load().earhip_allo_excluded_channels(self.h, len(zones), _zones(zones), C.byref(mask)))
        return mask.value

    def calculate(self, x, y, z, gain=None, diffuse=None, excluded=None):
        """Cartesian positions -> (direct, diffuse) float32 [n][n_channels] on the calling thread (no device needed); arrays
        [n] or scalars, None = absent (gain 1, diffuse 0, nothing excluded).  Raises on the first element the host form
        refuses, the message naming it; the rows before it are written (the exception's `partial`: the two arrays)."""
        f64 = C.POINTER(C.c_double)
        x = np.ascontiguousarray(np.atleast_1d(x), np.float64)
        n = x.size

        def arr(v, dtype=np.float64):
            return None if v is None else np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype), (n,)))
        y, z, gain, diffuse = arr(y), arr(z), arr(gain), arr(diffuse)
        excluded = arr(excluded, np.uint32)
        direct = np.full((n, self.n_out), np.nan, np.float32)
        diff = np.full((n, self.n_out), np.nan, np.float32)
        try:
            check(load().earhip_allo_calculate(self.h, C.c_size_t(n), _ptr(x, f64), _ptr(y, f64), _ptr(z, f64),
                                               None if gain is None else _ptr(gain, f64),
                                               None if diffuse is None else _ptr(diffuse, f64),
                                               None if excluded is None else _ptr(excluded, C.POINTER(C.c_uint32)),
                                               _ptr(direct), _ptr(diff)))
        except EarHipError as e:
            e.partial = (direct, diff)
            raise
        return direct, diff

    def lock_priority(self):
        """(U) the channel indices of the loudspeakers that are not LFE in the order a channelLock tie is resolved in"""
        n_real = int(np.count_nonzero(~np.isnan(self.positions()[:, 0])))
        order = np.zeros(n_real, np.int32)
        check(load().earhip_allo_lock_priority(self.h, _ptr(order, C.POINTER(C.c_int))))
        return [int(c) for c in order]

    def calculate_objects(self, x, y, z, width=None, height=None, depth=None, gain=None, diffuse=None, channel_lock=None,
                          lock_max_distance=None, divergence=None, position_range=None, excluded=None):
        """(U) Cartesian positions with extent, channelLock and divergence -> (direct, diffuse) float32 [n][n_channels] on
        the calling thread; arrays [n] or scalars, None = absent (sizes 0, gain 1, diffuse 0, no lock, no maxDistance,
        divergence 0, positionRange 0, nothing excluded).  Raises on the first element the host form refuses, the message
        naming it; the rows before it are written (the exception's `partial`: the two arrays)."""
        f64 = C.POINTER(C.c_double)
        x = np.ascontiguousarray(np.atleast_1d(x), np.float64)
        n = x.size

        def arr(v, dtype=np.float64, t=f64):
            if v is None:
                return None, None
            a = np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype), (n,)))
            return a, _ptr(a, t)
        ins = [arr(v) for v in (x, y, z, width, height, depth, gain, diffuse)]
        ins.append(arr(None if channel_lock is None else np.asarray(channel_lock) != 0, np.uint8, C.POINTER(C.c_ubyte)))
        ins += [arr(v) for v in (lock_max_distance, divergence, position_range)]
        ins.append(arr(excluded, np.uint32, C.POINTER(C.c_uint32)))
        direct = np.full((n, self.n_out), np.nan, np.float32)
        diff = np.full((n, self.n_out), np.nan, np.float32)
        try:
            check(load().earhip_allo_calculate_objects(self.h, C.c_size_t(n), *(p for _, p in ins), _ptr(direct), _ptr(diff)))
        except EarHipError as e:
            e.partial = (direct, diff)
            raise
        return direct, diff

    def close(self):
        if self.h:
            load().earhip_allo_destroy(self.h)
            self.h = C.c_void_p()


def allo_calculate_device(ctx, allo, n, x, y, z, gain, diffuse, excluded, direct, diffuse_out, status=None):
    """the same on the device: float64 tensors (or device addresses) of n elements, gain / diffuse / excluded (an int32
    tensor holding the mask bits) may be None, direct and diffuse_out float32 tensors [n][n_channels] (diffuse_out may be
    None when diffuse is), status an int32 tensor [n] (may be None): 1 and rows of NaN for an element Allo.calculate
    refuses.  Enqueues one kernel on the context's stream and does not synchronise."""
    nc = allo.n_out
    check(load().earhip_allo_calculate_device(ctx.h, allo.h, C.c_size_t(n), _dev_ptr(x, n, "float64"), _dev_ptr(y, n, "float64"),
                                              _dev_ptr(z, n, "float64"), _dev_ptr(gain, n, "float64"),
                                              _dev_ptr(diffuse, n, "float64"), _dev_ptr(excluded, n, "int32"),
                                              _dev_ptr(direct, n * nc, "float32"), _dev_ptr(diffuse_out, n * nc, "float32"),
                                              _dev_ptr(status, n, "int32")))


def allo_calculate_objects_device(ctx, allo, n, x, y, z, width, height, depth, gain, diffuse, channel_lock, lock_max_distance,
                                  divergence, position_range, excluded, direct, diffuse_out, status=None):
    """(U) Allo.calculate_objects on the device: float64 tensors (or device addresses) of n elements, channel_lock a uint8
    tensor, excluded an int32 tensor holding the mask bits; every input but x, y, z may be None; direct and diffuse_out
    float32 tensors [n][n_channels] (diffuse_out may be None when diffuse is), status an int32 tensor [n] (may be None): 1
    and rows of NaN for an element Allo.calculate_objects refuses.  Enqueues one kernel on the context's stream and does not
    synchronise."""
    nc = allo.n_out
    f64 = [_dev_ptr(v, n, "float64") for v in (x, y, z, width, height, depth, gain, diffuse)]
    check(load().earhip_allo_calculate_objects_device(
        ctx.h, allo.h, C.c_size_t(n), *f64, _dev_ptr(channel_lock, n, "uint8"), _dev_ptr(lock_max_distance, n, "float64"),
        _dev_ptr(divergence, n, "float64"), _dev_ptr(position_range, n, "float64"), _dev_ptr(excluded, n, "int32"),
        _dev_ptr(direct, n * nc, "float32"), _dev_ptr(diffuse_out, n * nc, "float32"), _dev_ptr(status, n, "int32")))


PCM_S16, PCM_S24, PCM_S32, PCM_F32 = 1, 2, 3, 4
_PCM = {"s16": (PCM_S16, np.int16, 1), "s24": (PCM_S24, np.uint8, 3), "s32": (PCM_S32, np.int32, 1),
        "f32": (PCM_F32, np.float32, 1)}
_PCM_BY_CODE = {v[0]: k for k, v in _PCM.items()}


def pcm_format(fmt):
    """(code, numpy dtype, array columns per channel) of a PCM format given as 's16' / 's24' / 's32' / 'f32' or its code"""
    name = _PCM_BY_CODE.get(fmt, fmt)
    if name not in _PCM:
        raise ValueError(f"unknown PCM format {fmt!r}")
    return _PCM[name]


# (W) the block timeline: audioBlockFormat timing -> the points of a renderer's curves (pure host functions)

TIMELINE_INTERPOLATED, TIMELINE_STEPPED = 0, 1
INT64_MIN, INT64_MAX = -2 ** 63, 2 ** 63 - 1
# earhip_block_timing
BLOCK_TIMING = np.dtype([("rtime", "<i8"), ("duration", "<i8"), ("interpolation_length", "<i8"), ("jump_position", "<i4")],
                        align=True)


def block_timings(blocks):
    """an earhip_block_timing array: from one (an array of dtype BLOCK_TIMING, used as it is), or from a sequence of
    (rtime, duration[, jump_position[, interpolation_length]]) in samples; duration -1 is an open end"""
    if isinstance(blocks, np.ndarray) and blocks.dtype == BLOCK_TIMING:
        return np.ascontiguousarray(blocks)
    out = np.zeros(len(blocks), BLOCK_TIMING)
    out["interpolation_length"] = -1
    for i, b in enumerate(blocks):
        out["rtime"][i], out["duration"][i] = b[0], b[1]
        if len(b) > 2:
            out["jump_position"][i] = b[2]
        if len(b) > 3:
            out["interpolation_length"][i] = b[3]
    return out


def timeline_window(mode, start, blocks, t0=INT64_MIN, t1=INT64_MAX):
    """(first, last) block whose rows the curve of the window [t0, t1) uses (include/earhip.h: earhip_timeline_window)"""
    b = block_timings(blocks)
    first, last = C.c_int(0), C.c_int(0)
    check(load().earhip_timeline_window(C.c_int(mode), C.c_int64(start), C.c_int(len(b)), C.c_void_p(b.ctypes.data),
                                        C.c_int64(t0), C.c_int64(t1), C.byref(first), C.byref(last)))
    return first.value, last.value


def timeline_points(mode, start, blocks, t0=INT64_MIN, t1=INT64_MAX):
    """(times int64 [n], source int32 [n]) of the window [t0, t1): source[k] is the block whose row of gains point k takes, -1
    the zero row (include/earhip.h: earhip_timeline_points, called once to count and once to fill)"""
    b = block_timings(blocks)
    args = (C.c_int(mode), C.c_int64(start), C.c_int(len(b)), C.c_void_p(b.ctypes.data), C.c_int64(t0), C.c_int64(t1))
    n = C.c_int(0)
    check(load().earhip_timeline_points(*args, C.c_int(0), None, None, C.byref(n)))
    times, source = np.empty(n.value, np.int64), np.empty(n.value, np.int32)
    check(load().earhip_timeline_points(*args, n, C.c_void_p(times.ctypes.data), C.c_void_p(source.ctypes.data), C.byref(n)))
    return times, source


class Renderer:
    """(F) composed Objects render block."""

    def __init__(self, ctx, n_objects, n_out, block_size, decorrelators=None, delay=0, max_blocks=1):
        self.ctx = ctx
        self.M, self.N, self.B = n_objects, n_out, block_size
        self.K = 2 if decorrelators is not None else 1
        cfg = RenderConfig()
        cfg.n_objects, cfg.n_out, cfg.block_size, cfg.n_buses = n_objects, n_out, block_size, self.K
        if decorrelators is not None:
            self._dec = _f32(decorrelators).reshape(n_out, -1)
            cfg.decorrelators = _ptr(self._dec)
            cfg.n_taps = self._dec.shape[1]
        else:
            cfg.decorrelators = None
            cfg.n_taps = 0
        cfg.delay = delay
        cfg.max_blocks = max_blocks
        self.h = C.c_void_p()
        check(load().earhip_render_create(ctx.h, C.byref(cfg), C.byref(self.h)))

    def set_object_points(self, obj, times, direct, diffuse=None):
        t = np.ascontiguousarray(times, dtype=np.int64)
        d = _f32(direct).reshape(len(t), self.N)
        f = _f32(diffuse).reshape(len(t), self.N) if diffuse is not None else None
        check(load().earhip_render_set_object_points(self.h, obj, len(t), _ptr(t, i64p), _ptr(d),
                                                     _ptr(f) if f is not None else None))

    def set_object_blocks(self, obj, mode, start, blocks, direct, diffuse=None, t0=INT64_MIN, t1=INT64_MAX):
        """one object's curve from its blocks' timing and one row of gains per block, direct / diffuse [n_blocks][n_out] in
        block order, for the window [t0, t1) (include/earhip.h group W: earhip_render_set_object_blocks)"""
        b = block_timings(blocks)
        d = _f32(direct).reshape(len(b), self.N)
        f = _f32(diffuse).reshape(len(b), self.N) if diffuse is not None else None
        check(load().earhip_render_set_object_blocks(self.h, C.c_int(obj), C.c_int(mode), C.c_int64(start), C.c_int(len(b)),
                                                     C.c_void_p(b.ctypes.data), C.c_int64(t0), C.c_int64(t1), _ptr(d),
                                                     _ptr(f) if f is not None else None))

    def set_objects_blocks(self, objects, modes, starts, block_offsets, blocks, direct, diffuse=None, t0=INT64_MIN, t1=INT64_MAX):
        """the curves of many objects in one call: track k is object objects[k] with blocks block_offsets[k] ..
        block_offsets[k + 1] of `blocks`; direct / diffuse [total blocks][n_out], the rows of a batch producer for the
        concatenated blocks.  Every track is checked before any curve changes (earhip_render_set_objects_blocks)."""
        o = np.ascontiguousarray(objects, dtype=np.int32)
        m = np.ascontiguousarray(modes, dtype=np.int32)
        s = np.ascontiguousarray(starts, dtype=np.int64)
        ofs = np.ascontiguousarray(block_offsets, dtype=np.int64)
        assert len(m) == len(o) and len(s) == len(o) and len(ofs) == len(o) + 1
        b = block_timings(blocks)
        assert len(o) == 0 or ofs[-1] <= len(b), "block_offsets reach beyond the blocks"
        d = _f32(direct).reshape(len(b), self.N)
        f = _f32(diffuse).reshape(len(b), self.N) if diffuse is not None else None
        check(load().earhip_render_set_objects_blocks(self.h, C.c_int(len(o)), C.c_void_p(o.ctypes.data), C.c_void_p(m.ctypes.data),
                                                      _ptr(s, i64p), _ptr(ofs, i64p), C.c_void_p(b.ctypes.data), C.c_int64(t0),
                                                      C.c_int64(t1), _ptr(d), _ptr(f) if f is not None else None))

    def commit(self):
        check(load().earhip_render_commit(self.h))

    def reset(self, sample_time=0):
        check(load().earhip_render_reset(self.h, C.c_int64(sample_time)))

    def process(self, x):
        """x [M][nblocks*B] host array -> [N][nblocks*B]."""
        x = _f32(x).reshape(self.M, -1)
        nblocks = x.shape[1] // self.B
        assert nblocks * self.B == x.shape[1]
        out = np.empty((self.N, x.shape[1]), np.float32)
        check(load().earhip_render_process(self.h, C.c_size_t(nblocks), _chan_ptrs(x), _chan_ptrs(out)))
        return out

    def process_into(self, x, out):
        """the same with the caller's own arrays, used as they are (e.g. Context.pinned_array: no staging copies)"""
        assert x.dtype == np.float32 and out.dtype == np.float32 and x.flags["C_CONTIGUOUS"] and out.flags["C_CONTIGUOUS"]
        nblocks = x.shape[1] // self.B
        assert x.shape == (self.M, nblocks * self.B) and out.shape == (self.N, nblocks * self.B)
        check(load().earhip_render_process(self.h, C.c_size_t(nblocks), _chan_ptrs(x), _chan_ptrs(out)))
        return out

    def process_device(self, nblocks, in_ptr, in_stride, out_ptr, out_stride):
        check(load().earhip_render_process_device(self.h, C.c_size_t(nblocks), C.c_void_p(in_ptr),
                                                  C.c_size_t(in_stride), C.c_void_p(out_ptr),
                                                  C.c_size_t(out_stride)))

    def _frames_shape(self, x, fmt):
        code, dtype, cols = pcm_format(fmt)
        assert x.dtype == dtype and x.ndim == 2 and x.flags["C_CONTIGUOUS"], (x.dtype, dtype, x.shape)
        assert x.shape[1] % cols == 0
        frames, channels = x.shape[0], x.shape[1] // cols
        nblocks = frames // self.B
        assert nblocks * self.B == frames, "frames must be whole blocks"
        return code, nblocks, channels

    def process_frames(self, x, fmt, first_channel=0, interleaved_out=False):
        """x [frames][C] interleaved PCM (int16 's16', int32 's32', float32 'f32'; uint8 [frames][3 C] 's24'), whole blocks;
        the renderer's inputs are channels [first_channel, first_channel + n_objects) -> [N][frames] float32, or [frames][N] with
        interleaved_out (include/earhip.h: earhip_render_process_frames)."""
        x = np.ascontiguousarray(x)
        frames = x.shape[0]
        out = np.empty((frames, self.N) if interleaved_out else (self.N, frames), np.float32)
        return self.process_frames_into(x, out, fmt, first_channel, interleaved_out)

    def process_frames_into(self, x, out, fmt, first_channel=0, interleaved_out=False):
        """the same with the caller's own arrays, used as they are (Context.pinned_array: DMA, no staging copies)"""
        code, nblocks, channels = self._frames_shape(x, fmt)
        frames = nblocks * self.B
        assert out.dtype == np.float32 and out.flags["C_CONTIGUOUS"]
        assert out.shape == ((frames, self.N) if interleaved_out else (self.N, frames)), out.shape
        ptrs = (f32p * 1)(_ptr(out)) if interleaved_out else _chan_ptrs(out)
        check(load().earhip_render_process_frames(self.h, C.c_size_t(nblocks), C.c_void_p(x.ctypes.data), C.c_int(code),
                                                  C.c_int(channels), C.c_int(first_channel), ptrs, int(bool(interleaved_out))))
        return out

    def process_frames_device(self, nblocks, frames_ptr, fmt, frame_channels, first_channel, out_ptr, out_stride,
                              interleaved_out=False):
        """device pointers (e.g. torch tensors' data_ptr()); enqueues on the context's stream"""
        code = pcm_format(fmt)[0] if isinstance(fmt, str) else int(fmt)
        check(load().earhip_render_process_frames_device(self.h, C.c_size_t(nblocks), C.c_void_p(frames_ptr), C.c_int(code),
                                                         C.c_int(frame_channels), C.c_int(first_channel), C.c_void_p(out_ptr),
                                                         C.c_size_t(out_stride), int(bool(interleaved_out))))

    def process_frames_pcm(self, x, fmt, first_channel=0, out_fmt="s16", dither=False, seed=0):
        """interleaved PCM frames in (as process_frames) -> interleaved PCM frames out, converted on the device: int16 's16' /
        int32 's32' / float32 'f32' [frames][N], or uint8 [frames][3 N] 's24'; dither: TPDF, 's16' only, a function of
        (seed, sample clock, channel) (include/earhip.h: earhip_render_process_frames_pcm)."""
        x = np.ascontiguousarray(x)
        _, dtype, cols = pcm_format(out_fmt)
        out = np.empty((x.shape[0], self.N * cols), dtype)
        return self.process_frames_pcm_into(x, out, fmt, first_channel, out_fmt, dither, seed)

    def process_frames_pcm_into(self, x, out, fmt, first_channel=0, out_fmt="s16", dither=False, seed=0):
        """the same with the caller's own arrays, used as they are (Context.pinned_array: DMA both ways, no staging copies)"""
        code, nblocks, channels = self._frames_shape(x, fmt)
        ocode, dtype, cols = pcm_format(out_fmt)
        assert out.dtype == dtype and out.flags["C_CONTIGUOUS"] and out.shape == (nblocks * self.B, self.N * cols), out.shape
        spec = PcmOut(ocode, int(dither), int(seed) & 0xFFFFFFFF)
        check(load().earhip_render_process_frames_pcm(self.h, C.c_size_t(nblocks), C.c_void_p(x.ctypes.data), C.c_int(code),
                                                      C.c_int(channels), C.c_int(first_channel), C.c_void_p(out.ctypes.data),
                                                      C.byref(spec)))
        return out

    def process_frames_pcm_device(self, nblocks, frames_ptr, fmt, frame_channels, first_channel, out_ptr, out_frame_bytes,
                                  out_first_byte=0, out_fmt="s16", dither=False, seed=0):
        """device pointers; the renderer's samples are bytes [out_first_byte, + N * sample size) of each output frame of
        out_frame_bytes, every other byte is left alone; enqueues on the context's stream"""
        code = pcm_format(fmt)[0] if isinstance(fmt, str) else int(fmt)
        ocode = pcm_format(out_fmt)[0] if isinstance(out_fmt, str) else int(out_fmt)
        spec = PcmOut(ocode, int(dither), int(seed) & 0xFFFFFFFF)
        check(load().earhip_render_process_frames_pcm_device(self.h, C.c_size_t(nblocks), C.c_void_p(frames_ptr), C.c_int(code),
                                                             C.c_int(frame_channels), C.c_int(first_channel), C.c_void_p(out_ptr),
                                                             C.c_size_t(out_frame_bytes), C.c_size_t(out_first_byte),
                                                             C.byref(spec)))

    def output_levels(self, reset=False):
        """(peak float32 [N], clipped uint64 [N]) of the samples that went through the PCM-out calls since these numbers were
        last zeroed (reset=True zeroes them afterwards; so does reset()): the largest |x| and the saturated samples"""
        peak, clipped = np.zeros(self.N, np.float32), np.zeros(self.N, np.uint64)
        check(load().earhip_render_output_levels(self.h, _ptr(peak), C.c_void_p(clipped.ctypes.data), int(bool(reset))))
        return peak, clipped

    def enable_timing(self, on=True):
        """True / 1: time the kernels of every process call; n > 1: of every n-th call; False: stop"""
        check(load().earhip_render_enable_timing(self.h, int(on)))

    def get_timing(self):
        out = (C.c_double * 6)()
        check(load().earhip_render_get_timing(self.h, out))
        return {"gain_mix_ms": out[0], "gain_mix_launches": out[1], "decor_ms": out[2],
                "decor_launches": out[3], "prep_ms": out[4], "prep_launches": out[5]}

    def gain_kernel(self):
        """0 strict VALU, 1 f32 MFMA (slot lists), 2 f32 MFMA on the tile grid, 3 f16x2 MFMA, 4 f16x2 MFMA over piece lists, 5 f16x2 MFMA
        with hinges: the gain kernel of
        the last call"""
        kind = C.c_int(-1)
        check(load().earhip_render_gain_kernel(self.h, C.byref(kind)))
        return kind.value

    def hinge_standby(self):
        """True when the last call was planned for the hinge kernel (5) and the device handed it to the piece lists standing
        by (its inputs' levels spread further than the hinge kernel's span); synchronises the stream"""
        flag = C.c_int(0)
        check(load().earhip_render_hinge_standby(self.h, C.byref(flag)))
        return bool(flag.value)

    def hinge_robust(self):
        """True when the last call was the hinge kernel's (5) and ran its robust form: kink products in f32, because the levels of
        the call's inputs spread beyond the span of the packed-f16 products (earhip_render_hinge_robust); synchronises the stream"""
        flag = C.c_int(0)
        check(load().earhip_render_hinge_robust(self.h, C.byref(flag)))
        return bool(flag.value)

    def wide_form(self):
        """True / False: the form (wide / plain low pieces of the inputs) the split-operand kernel of the last call ran — picked on
        the device for long calls, wide for short ones; None when the kernel has no split operands; synchronises the stream"""
        flag = C.c_int(1)
        check(load().earhip_render_wide_form(self.h, C.byref(flag)))
        return None if flag.value < 0 else bool(flag.value)

    def scratch_bytes(self):
        """device scratch (descriptors, lists) the last call needed"""
        v = C.c_size_t(0)
        check(load().earhip_render_scratch_bytes(self.h, C.byref(v)))
        return v.value

    def scratch_regrows(self):
        """process calls that had to grow the list scratch themselves (0 on committed curves)"""
        v = C.c_long(0)
        check(load().earhip_render_scratch_regrows(self.h, C.byref(v)))
        return v.value

    def last_tail_blocks(self):
        """blocks of the last call that ran as a tail of their own behind the whole rounds of tiles (0: the call was not cut)"""
        v = C.c_int(0)
        check(load().earhip_render_last_tail_blocks(self.h, C.byref(v)))
        return v.value

    def last_host_chunks(self):
        """time chunks the last call from host channel pointers ran as (0: one piece)"""
        v = C.c_int(0)
        check(load().earhip_render_last_host_chunks(self.h, C.byref(v)))
        return v.value

    def last_list_layout(self):
        """layout of the last call's piece lists: True paired, False packed, None: none built"""
        v = C.c_int(0)
        check(load().earhip_render_last_list_layout(self.h, C.byref(v)))
        return None if v.value < 0 else bool(v.value)

    def last_plan(self):
        """launch plan of the last call: gain kernel, samples per workgroup tile, tiles, object splits"""
        out = (C.c_int * 4)()
        check(load().earhip_render_last_plan(self.h, out))
        return {"kernel": out[0], "tile": out[1], "ntiles": out[2], "gsplit": out[3]}

    def last_decor_plan(self):
        """the decorrelator stage's plan: partition size and count of the FIRs, and of the last call the kernel form (0 workgroup
        kernel of a fixed size, 1 run-time shape, 2 wave kernel) and the blocks per run; zeros on one bus"""
        out = (C.c_int * 4)()
        check(load().earhip_render_last_decor_plan(self.h, out))
        return {"Bk": out[0], "NP": out[1], "form": out[2], "run": out[3]}

    def attach_loudness(self, meter):
        """every process call of every form feeds its float32 output samples to `meter` (a Loudness of n_out channels on this
        context) on the device; None detaches (include/earhip.h: earhip_render_attach_loudness)"""
        check(load().earhip_render_attach_loudness(self.h, meter.h if meter is not None else None))
        self._meter = meter  # (kept alive while attached)

    def attach_fir_matrix(self, fm, sink_ptr=None, sink_stride=0, sink_capacity=0):
        """every process call of every form feeds its float32 output rows to `fm` (a FirMatrix with n_in = n_out of this
        renderer, its block size and its context) on the device; fm's rows go to sink_ptr[k * sink_stride + position] (device
        memory or a Context.pinned_array's address); None detaches (include/earhip.h: earhip_render_attach_firmix)"""
        check(load().earhip_render_attach_firmix(self.h, fm.h if fm is not None else None,
                                                 C.c_void_p(sink_ptr) if sink_ptr else None, C.c_size_t(sink_stride),
                                                 C.c_size_t(sink_capacity)))
        self._fir_matrix = fm  # (kept alive while attached)

    def fir_matrix_position(self):
        """samples fed to the attached FirMatrix since the attach = where its next row samples go in the sink"""
        v = C.c_size_t(0)
        check(load().earhip_render_firmix_position(self.h, C.byref(v)))
        return v.value

    def attach_limiter(self, lim, sink_ptr=None, sink_stride=0, sink_capacity=0):
        """every process call of every form feeds its float32 output rows to `lim` (a Limiter of n_out channels on this context)
        on the device, behind an attached meter and FIR matrix, which keep seeing the unlimited bus; the limited rows go to
        sink_ptr[c * sink_stride + position]; None detaches (include/earhip.h: earhip_render_attach_limiter)"""
        check(load().earhip_render_attach_limiter(self.h, lim.h if lim is not None else None,
                                                  C.c_void_p(sink_ptr) if sink_ptr else None, C.c_size_t(sink_stride),
                                                  C.c_size_t(sink_capacity)))
        self._limiter = lim  # (kept alive while attached)

    def limiter_position(self):
        """samples fed to the attached Limiter since the attach = where its next row samples go in the sink"""
        v = C.c_size_t(0)
        check(load().earhip_render_limiter_position(self.h, C.byref(v)))
        return v.value

    def close(self):
        if self.h:
            load().earhip_render_destroy(self.h)
            self.h = C.c_void_p()


# (L) programme loudness, ITU-R BS.1770-4

def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def loudness_gate(energy, weights):
    """step energies [steps][channels] (Loudness.steps; the columns of several meters side by side) and channel weights ->
    (integrated, max momentary, max short-term) in LKFS, -inf where undefined; on the calling thread, no device"""
    w = _f64(weights).reshape(-1)
    e = _f64(energy).reshape(-1, w.size)
    out = [C.c_double(0) for _ in range(3)]
    check(load().earhip_loudness_gate(C.c_size_t(e.shape[0]), C.c_int(w.size), C.c_void_p(e.ctypes.data), C.c_void_p(w.ctypes.data),
                                      *[C.byref(v) for v in out]))
    return tuple(v.value for v in out)


def loudness_range(energy, weights):
    """step energies [steps][channels] and channel weights -> (LRA in LU, low, high in LKFS) by EBU Tech 3342; (0, -inf, -inf)
    where no short-term window survives the gates; on the calling thread, no device"""
    w = _f64(weights).reshape(-1)
    e = _f64(energy).reshape(-1, w.size)
    out = [C.c_double(0) for _ in range(3)]
    check(load().earhip_loudness_range(C.c_size_t(e.shape[0]), C.c_int(w.size), C.c_void_p(e.ctypes.data), C.c_void_p(w.ctypes.data),
                                       *[C.byref(v) for v in out]))
    return tuple(v.value for v in out)


class _TruePeak(C.Structure):
    _fields_ = [("phases", C.c_int), ("taps", C.c_int), ("coeffs", C.c_void_p)]


def loudness_layout_weights(layout):
    """BS.1770-4's channel weights of a BS.2051 layout, float64 [channels of the full layout] (LFE channels 0)"""
    n = C.c_int(0)
    check(load().earhip_layout_num_channels(layout.encode(), C.byref(n)))
    w = np.zeros(n.value, np.float64)
    check(load().earhip_loudness_layout_weights(layout.encode(), C.c_void_p(w.ctypes.data)))
    return w


class _BusStage:
    """what the output-bus stages share: the handle `h` of earhip_<_stem>_create goes back through earhip_<_stem>_reset and
    earhip_<_stem>_destroy"""
    _stem = None

    def reset(self):
        check(getattr(load(), f"earhip_{self._stem}_reset")(self.h))

    def close(self):
        if self.h:
            getattr(load(), f"earhip_{self._stem}_destroy")(self.h)
            self.h = C.c_void_p()


class Loudness(_BusStage):
    """(L) the meter: K-weighted 100 ms step energies kept on the device, gated on request.  true_peak=True also measures
    true and sample peak with BS.1770-4's 4 x 12 interpolator (44100 and 48000 Hz); (phases, taps, coeffs [phases][taps]) brings
    another table."""
    _stem = "loudness"

    def __init__(self, ctx, n_channels, sample_rate=48000, max_steps=36000, coeffs=None, true_peak=False):
        self.ctx, self.C = ctx, n_channels
        c = None if coeffs is None else _f64(coeffs).reshape(2, 5)
        self.h = C.c_void_p()
        kc = None if c is None else C.c_void_p(c.ctypes.data)
        if true_peak is False or true_peak is None:
            check(load().earhip_loudness_create(ctx.h, C.c_int(n_channels), C.c_int(sample_rate), kc, C.c_size_t(max_steps),
                                                C.byref(self.h)))
            return
        if true_peak is True:
            tp = _TruePeak(0, 0, None)
        else:
            phases, taps, table = true_peak
            table = _f64(table).reshape(-1)
            if table.size != max(int(phases), 0) * max(int(taps), 0):
                raise InvalidArgument(INVALID_ARGUMENT, "the true-peak table must be [phases][taps]")
            if table.size == 0:
                table = np.zeros(1)  # (a table, not the default: the library refuses its shape)
            tp = _TruePeak(int(phases), int(taps), table.ctypes.data)
        check(load().earhip_loudness_create_tp(ctx.h, C.c_int(n_channels), C.c_int(sample_rate), kc, C.c_size_t(max_steps),
                                               C.byref(tp), C.byref(self.h)))

    def process(self, x):
        """x [channels][n] host array, any n"""
        x = _f32(x).reshape(self.C, -1)
        check(load().earhip_loudness_process(self.h, C.c_size_t(x.shape[1]), _chan_ptrs(x)))

    def process_device(self, nsamples, rows_ptr, stride):
        """planar float32 rows in device memory (e.g. a torch tensor's data_ptr()); enqueues on the context's stream"""
        check(load().earhip_loudness_process_device(self.h, C.c_size_t(nsamples), C.c_void_p(rows_ptr), C.c_size_t(stride)))

    def num_steps(self):
        v = C.c_size_t(0)
        check(load().earhip_loudness_num_steps(self.h, C.byref(v)))
        return v.value

    def steps(self, first=0, n=None):
        """step energies [n][channels] float64 of the finished steps [first, first + n) (default: all from first)"""
        if n is None:
            n = self.num_steps() - first
        e = np.zeros((n, self.C), np.float64)
        check(load().earhip_loudness_steps(self.h, C.c_size_t(first), C.c_size_t(n), C.c_void_p(e.ctypes.data)))
        return e

    def result(self, weights):
        """(integrated, max momentary, max short-term) in LKFS over all finished steps"""
        w = _f64(weights).reshape(self.C)
        out = [C.c_double(0) for _ in range(3)]
        check(load().earhip_loudness_result(self.h, C.c_void_p(w.ctypes.data), *[C.byref(v) for v in out]))
        return tuple(v.value for v in out)

    def peaks(self):
        """(true peak [channels], sample peak [channels]) so far, linear float32, the unfinished step included"""
        t, s = np.zeros(self.C, np.float32), np.zeros(self.C, np.float32)
        check(load().earhip_loudness_peaks(self.h, C.c_void_p(t.ctypes.data), C.c_void_p(s.ctypes.data)))
        return t, s

    def step_peaks(self, first=0, n=None):
        """(true peak, sample peak), [n][channels] float32 each, of the finished steps [first, first + n) (default: all from first)"""
        if n is None:
            n = self.num_steps() - first
        t, s = np.zeros((n, self.C), np.float32), np.zeros((n, self.C), np.float32)
        check(load().earhip_loudness_step_peaks(self.h, C.c_size_t(first), C.c_size_t(n), C.c_void_p(t.ctypes.data),
                                                C.c_void_p(s.ctypes.data)))
        return t, s

    def range(self, weights):
        """(LRA in LU, low, high in LKFS) over all finished steps (EBU Tech 3342)"""
        w = _f64(weights).reshape(self.C)
        out = [C.c_double(0) for _ in range(3)]
        check(load().earhip_loudness_result_range(self.h, C.c_void_p(w.ctypes.data), *[C.byref(v) for v in out]))
        return tuple(v.value for v in out)


# (M) FIR filter matrix

class _FirmixConfig(C.Structure):
    _fields_ = [("n_in", C.c_int), ("n_out", C.c_int), ("block_size", C.c_int), ("n_taps", C.c_int), ("taps", C.c_void_p),
                ("max_blocks", C.c_int)]


class FirMatrix(_BusStage):
    """(M) taps [K][C][J] float32: K outputs from C inputs through one J-tap FIR per pair, partitioned at block_size; pairs whose
    taps are all zero cost nothing and their input channels are never read.  n_sets: room for that many filter sets of this shape
    (earhip_firmix_create_sets: `taps` is set 0 and current; load_set / select switch and crossfade while it runs); None: a plain
    matrix (earhip_firmix_create)."""
    _stem = "firmix"

    def __init__(self, ctx, taps, block_size, max_blocks=1, n_sets=None):
        taps = _f32(taps)
        if taps.ndim != 3:
            raise InvalidArgument(INVALID_ARGUMENT, "taps must be [n_out][n_in][n_taps]")
        if n_sets is not None and (isinstance(n_sets, bool) or not isinstance(n_sets, (int, np.integer))):
            raise InvalidArgument(INVALID_ARGUMENT, "n_sets must be an integer or None")
        self.ctx = ctx
        self.K, self.C, self.J = (int(v) for v in taps.shape)
        self.B = int(block_size)
        cfg = _FirmixConfig(self.C, self.K, self.B, self.J, taps.ctypes.data if taps.size else None, int(max_blocks))
        self.h = C.c_void_p()
        self.n_sets = None if n_sets is None else int(n_sets)
        if n_sets is None:
            check(load().earhip_firmix_create(ctx.h, C.byref(cfg), C.byref(self.h)))
        else:
            check(load().earhip_firmix_create_sets(ctx.h, C.byref(cfg), C.c_int(self.n_sets), C.byref(self.h)))

    def load_set(self, index, taps):
        """host taps [K][C][J] become set `index` (not the current set, nor one being faded from); enqueues the transforms"""
        taps = _f32(taps)
        if taps.shape != (self.K, self.C, self.J):
            raise InvalidArgument(INVALID_ARGUMENT, "taps must have the shape the matrix was made with")
        check(load().earhip_firmix_load_set(self.h, C.c_int(int(index)), C.c_void_p(taps.ctypes.data)))

    def load_set_device(self, index, taps_ptr):
        """the same from float32 [K][C][J] in device memory (e.g. a torch tensor's data_ptr()): no pair is dropped, nothing is
        allocated or synchronised"""
        if not taps_ptr:
            raise InvalidArgument(INVALID_ARGUMENT, "taps_ptr must not be NULL")
        check(load().earhip_firmix_load_set_device(self.h, C.c_int(int(index)), C.c_void_p(taps_ptr)))

    def select(self, index, fade_blocks=0):
        """from the next block fed, go to set `index` over fade_blocks blocks (0: a hard switch): host bookkeeping only"""
        check(load().earhip_firmix_select(self.h, C.c_int(int(index)), C.c_int(int(fade_blocks))))

    def state(self):
        out = (C.c_int * 4)()
        check(load().earhip_firmix_state(self.h, out))
        return {"current": out[0], "from": out[1], "done": out[2], "total": out[3]}

    def set_info(self, index):
        out = (C.c_int * 2)()
        check(load().earhip_firmix_set_info(self.h, C.c_int(int(index)), out))
        return {"loaded": bool(out[0]), "pairs": out[1]}

    def process(self, x):
        """x [C][nblocks * B] host array -> [K][nblocks * B]"""
        x = _f32(x).reshape(self.C, -1)
        nblocks = x.shape[1] // self.B
        assert nblocks * self.B == x.shape[1], "whole blocks"
        out = np.empty((self.K, x.shape[1]), np.float32)
        check(load().earhip_firmix_process(self.h, C.c_size_t(nblocks), _chan_ptrs(x), _chan_ptrs(out)))
        return out

    def process_device(self, nblocks, in_ptr, in_stride, out_ptr, out_stride):
        """planar float32 rows in device memory (e.g. torch tensors' data_ptr()); enqueues on the context's stream"""
        check(load().earhip_firmix_process_device(self.h, C.c_size_t(nblocks), C.c_void_p(in_ptr), C.c_size_t(in_stride),
                                                  C.c_void_p(out_ptr), C.c_size_t(out_stride)))

    def info(self):
        out = (C.c_int * 5)()
        check(load().earhip_firmix_info(self.h, out))
        return {"n_in": out[0], "n_out": out[1], "block_size": out[2], "partitions": out[3], "pairs": out[4]}


# (N) look-ahead true-peak limiter

class _LimiterConfig(C.Structure):
    _fields_ = [("n_channels", C.c_int), ("sample_rate", C.c_int), ("ceiling", C.c_float), ("lookahead", C.c_int),
                ("hold", C.c_int), ("detect", C.c_int), ("tp", C.c_void_p), ("max_samples", C.c_size_t)]


class Limiter(_BusStage):
    """(N) one gain for all channels that keeps every output sample under `ceiling`, looking `lookahead` samples ahead and
    holding `hold` samples; true_peak=True detects on BS.1770-4's 4 x 12 interpolator (44100 and 48000 Hz), (phases, taps,
    coeffs [phases][taps]) brings another table, False detects sample peaks only.  The output is delayed by latency() samples."""
    _stem = "limiter"

    def __init__(self, ctx, n_channels, ceiling, lookahead=64, hold=480, sample_rate=48000, true_peak=True, max_samples=48000):
        for name, v in (("n_channels", n_channels), ("lookahead", lookahead), ("hold", hold), ("sample_rate", sample_rate),
                        ("max_samples", max_samples)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise InvalidArgument(INVALID_ARGUMENT, f"{name} must be an integer")
        if int(max_samples) < 0:
            raise InvalidArgument(INVALID_ARGUMENT, "max_samples must be >= 1")
        self.ctx, self.C = ctx, int(n_channels)
        self.max_samples = int(max_samples)
        tp = None
        if true_peak is not True and true_peak is not False and true_peak is not None:
            phases, taps, table = true_peak
            table = _f64(table).reshape(-1)
            if table.size != max(int(phases), 0) * max(int(taps), 0):
                raise InvalidArgument(INVALID_ARGUMENT, "the true-peak table must be [phases][taps]")
            if table.size == 0:
                table = np.zeros(1)  # (a table, not the default: the library refuses its shape)
            self._table = table
            tp = _TruePeak(int(phases), int(taps), table.ctypes.data)
        cfg = _LimiterConfig(self.C, int(sample_rate), float(ceiling), int(lookahead), int(hold), 1 if true_peak else 0,
                             C.cast(C.pointer(tp), C.c_void_p) if tp is not None else None, self.max_samples)
        self.h = C.c_void_p()
        check(load().earhip_limiter_create(ctx.h if ctx is not None else None, C.byref(cfg), C.byref(self.h)))

    def latency(self):
        v = C.c_int(0)
        check(load().earhip_limiter_latency(self.h, C.byref(v)))
        return v.value

    def process(self, x, with_gain=False):
        """x [channels][n] host array, any n -> the limited rows [channels][n] (and the gain row [n])"""
        x = _f32(x)
        if x.ndim != 2 or x.shape[0] != self.C:
            raise InvalidArgument(INVALID_ARGUMENT, "x must be [channels][n]")
        n = x.shape[1]
        out = np.empty((self.C, n), np.float32)
        g = np.empty(n, np.float32) if with_gain else None
        check(load().earhip_limiter_process(self.h, C.c_size_t(n), _chan_ptrs(x), _chan_ptrs(out), _ptr(g) if with_gain else None))
        return (out, g) if with_gain else out

    def process_device(self, nsamples, in_ptr, in_stride, out_ptr, out_stride, gain_ptr=None):
        """planar float32 rows in device memory (e.g. torch tensors' data_ptr()); gain_ptr: [nsamples] or None; enqueues on the
        context's stream"""
        check(load().earhip_limiter_process_device(self.h, C.c_size_t(nsamples), C.c_void_p(in_ptr), C.c_size_t(in_stride),
                                                   C.c_void_p(out_ptr), C.c_size_t(out_stride),
                                                   C.c_void_p(gain_ptr) if gain_ptr else None))

    def process_pcm_device(self, nsamples, in_ptr, in_stride, out_ptr, out_frame_bytes, out_first_byte=0, out_fmt="s16",
                           dither=False, seed=0):
        """the limited rows as PCM frames: bytes [out_first_byte, + channels * sample size) of each output frame of
        out_frame_bytes in device memory, every other byte is left alone; enqueues on the context's stream"""
        ocode = pcm_format(out_fmt)[0] if isinstance(out_fmt, str) else int(out_fmt)
        spec = PcmOut(ocode, int(dither), int(seed) & 0xFFFFFFFF)
        check(load().earhip_limiter_process_pcm_device(self.h, C.c_size_t(nsamples), C.c_void_p(in_ptr), C.c_size_t(in_stride),
                                                       C.c_void_p(out_ptr), C.c_size_t(out_frame_bytes),
                                                       C.c_size_t(out_first_byte), C.byref(spec)))

    def output_levels(self, reset=False):
        """(peak float32 [channels], clipped uint64 [channels]) of the samples that went through process_pcm_device"""
        peak, clipped = np.zeros(self.C, np.float32), np.zeros(self.C, np.uint64)
        check(load().earhip_limiter_output_levels(self.h, _ptr(peak), C.c_void_p(clipped.ctypes.data), int(bool(reset))))
        return peak, clipped

    def stats(self, reset=False):
        """(the smallest gain so far as numpy float32, the number of samples with a gain below 1)"""
        g, n = C.c_float(1.0), C.c_uint64(0)
        check(load().earhip_limiter_stats(self.h, C.byref(g), C.byref(n), int(bool(reset))))
        return np.float32(g.value), n.value


# (O) biquad filter matrix

IIR_KINDS = {"lowpass": 0, "highpass": 1, "peaking": 2, "low_shelf": 3, "high_shelf": 4}


class _IirRoute(C.Structure):
    _fields_ = [("in_", C.c_int), ("out", C.c_int), ("gain", C.c_double), ("n_sections", C.c_int),
                ("coeffs", (C.c_double * 5) * 8)]


class _IirConfig(C.Structure):
    _fields_ = [("n_in", C.c_int), ("n_out", C.c_int), ("n_routes", C.c_int), ("routes", C.POINTER(_IirRoute)),
                ("max_samples", C.c_size_t)]


def iir_design(kind, sample_rate, f0, q=2.0 ** -0.5, gain_db=0.0):
    """one RBJ cookbook section [b0 b1 b2 a1 a2] (float64); kind: a name of IIR_KINDS or its number.  A pure host function"""
    out = np.zeros(5, np.float64)
    code = IIR_KINDS.get(kind, -1) if isinstance(kind, str) else int(kind)
    load().earhip_iir_design.argtypes = [C.c_int, C.c_double, C.c_double, C.c_double, C.c_double, C.c_void_p]
    check(load().earhip_iir_design(code, float(sample_rate), float(f0), float(q), float(gain_db), C.c_void_p(out.ctypes.data)))
    return out


class IirBank(_BusStage):
    """(O) a matrix of biquad cascades: routes = [(in, out, gain, sections)], sections [S][5] = b0 b1 b2 a1 a2 with S in
    [0, 8] (S = 0, or None: a pure gain route); out_k = the sum of gain * filtered input over the routes into k."""
    _stem = "iir"

    def __init__(self, ctx, n_in, n_out, routes, max_samples=48000):
        for name, v in (("n_in", n_in), ("n_out", n_out), ("max_samples", max_samples)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise InvalidArgument(INVALID_ARGUMENT, f"{name} must be an integer")
        if int(max_samples) < 1:
            raise InvalidArgument(INVALID_ARGUMENT, "max_samples must be >= 1")
        routes = list(routes)
        arr = (_IirRoute * max(len(routes), 1))()
        for i, route in enumerate(routes):
            if len(route) != 4:
                raise InvalidArgument(INVALID_ARGUMENT, "a route is (in, out, gain, sections)")
            rin, rout, gain, sections = route
            for name, v in (("in", rin), ("out", rout)):
                if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                    raise InvalidArgument(INVALID_ARGUMENT, f"a route's {name} must be an integer")
            sec = np.zeros((0, 5)) if sections is None else _f64(sections)
            if sec.size == 0:
                sec = sec.reshape(0, 5)
            if sec.ndim != 2 or sec.shape[1] != 5:
                raise InvalidArgument(INVALID_ARGUMENT, "a route's sections must be [S][5]")
            arr[i].in_, arr[i].out, arr[i].gain, arr[i].n_sections = int(rin), int(rout), float(gain), sec.shape[0]
            for s in range(min(sec.shape[0], 8)):
                for j in range(5):
                    arr[i].coeffs[s][j] = sec[s, j]
        self.ctx, self.n_in, self.n_out = ctx, int(n_in), int(n_out)
        self.max_samples = int(max_samples)
        cfg = _IirConfig(self.n_in, self.n_out, len(routes), arr, self.max_samples)
        self.h = C.c_void_p()
        check(load().earhip_iir_create(ctx.h if ctx is not None else None, C.byref(cfg), C.byref(self.h)))

    def info(self):
        """dict: chunk (Lc), scan_lanes, scan_groups, routes, max_state, scratch_bytes"""
        v = (C.c_int * 6)()
        check(load().earhip_iir_info(self.h, v))
        return dict(zip(("chunk", "scan_lanes", "scan_groups", "routes", "max_state", "scratch_bytes"), list(v)))

    def process(self, x):
        """x [n_in][n] host array, any n -> [n_out][n]"""
        x = _f32(x)
        if x.ndim != 2 or x.shape[0] != self.n_in:
            raise InvalidArgument(INVALID_ARGUMENT, "x must be [n_in][n]")
        n = x.shape[1]
        out = np.empty((self.n_out, n), np.float32)
        check(load().earhip_iir_process(self.h, C.c_size_t(n), _chan_ptrs(x), _chan_ptrs(out)))
        return out

    def process_device(self, nsamples, in_ptr, in_stride, out_ptr, out_stride):
        """planar float32 rows in device memory (e.g. torch tensors' data_ptr()); enqueues on the context's stream"""
        check(load().earhip_iir_process_device(self.h, C.c_size_t(nsamples), C.c_void_p(in_ptr), C.c_size_t(in_stride),
                                               C.c_void_p(out_ptr), C.c_size_t(out_stride)))


# (P) polyphase sample-rate converter

class _SrcConfig(C.Structure):
    _fields_ = [("channels", C.c_int), ("up", C.c_int), ("down", C.c_int), ("taps_per_phase", C.c_int),
                ("taps", C.c_void_p), ("max_samples", C.c_size_t)]


class _SrcProperties(C.Structure):
    _fields_ = [("up", C.c_int), ("down", C.c_int), ("taps_per_phase", C.c_int), ("tile_out", C.c_int), ("tile_in", C.c_int),
                ("table_in_lds", C.c_int), ("window_in_lds", C.c_int), ("max_out", C.c_size_t),
                ("latency_prototype", C.c_double), ("latency_in", C.c_double), ("latency_out", C.c_double)]


def _src_int(name, v):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
        raise InvalidArgument(INVALID_ARGUMENT, f"{name} must be an integer")
    if not -2 ** 31 <= int(v) < 2 ** 31:
        raise InvalidArgument(INVALID_ARGUMENT, f"{name} is out of range")
    return int(v)


def src_design(up, down, taps_per_phase, beta=10.0, cutoff=1.0):
    """the prototype h[up * taps_per_phase] (float64) of a rate change by up / down: a Kaiser-windowed sinc with its cutoff at
    cutoff / max(up, down) of the prototype's Nyquist, unit DC gain, times up.  A pure host function"""
    up, down, T = _src_int("up", up), _src_int("down", down), _src_int("taps_per_phase", taps_per_phase)
    out = np.zeros(max(up * T, 1) if 0 < up <= 1024 and 0 < T <= 256 else 1, np.float64)
    load().earhip_src_design.argtypes = [C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_void_p]
    check(load().earhip_src_design(up, down, T, float(beta), float(cutoff), C.c_void_p(out.ctypes.data)))
    return out


class SampleRateConverter(_BusStage):
    """(P) a rational rate change by up / down on planar float32 rows: y = scipy.signal.upfirdn(taps, x, up, down) in float32,
    every output one chain of taps_per_phase fused multiply-adds; the same bits however the stream is cut into calls."""
    _stem = "src"

    def __init__(self, ctx, channels, up, down, taps_per_phase, taps, max_samples=48000):
        channels, up, down = _src_int("channels", channels), _src_int("up", up), _src_int("down", down)
        T = _src_int("taps_per_phase", taps_per_phase)
        if isinstance(max_samples, bool) or not isinstance(max_samples, (int, np.integer)) or int(max_samples) < 1:
            raise InvalidArgument(INVALID_ARGUMENT, "max_samples must be an integer >= 1")
        h = np.ascontiguousarray(np.asarray(taps, np.float64).reshape(-1))
        if 0 < up <= 1024 and 0 < T <= 256 and h.size != up * T:
            raise InvalidArgument(INVALID_ARGUMENT, "taps must hold up * taps_per_phase values")
        self.ctx, self.channels, self.up, self.down, self.taps_per_phase = ctx, channels, up, down, T
        self.max_samples = int(max_samples)
        cfg = _SrcConfig(channels, up, down, T, C.c_void_p(h.ctypes.data) if h.size else None, self.max_samples)
        self.h = C.c_void_p()
        check(load().earhip_src_create(ctx.h if ctx is not None else None, C.byref(cfg), C.byref(self.h)))
        self.max_out = self.info()["max_out"]

    def info(self):
        """dict: up, down, taps_per_phase, tile_out, tile_in, table_in_lds, window_in_lds, max_out, latency_prototype /_in /_out"""
        v = _SrcProperties()
        check(load().earhip_src_info(self.h, C.byref(v)))
        return {name: getattr(v, name) for name, _ in _SrcProperties._fields_}

    def next_out(self, nsamples):
        """the outputs a call of nsamples inputs would produce now"""
        n = C.c_size_t(0)
        check(load().earhip_src_next_out(self.h, C.c_size_t(nsamples), C.byref(n)))
        return n.value

    def process(self, x):
        """x [channels][n] host array, any n -> [channels][n_out]"""
        x = _f32(x)
        if x.ndim != 2 or x.shape[0] != self.channels:
            raise InvalidArgument(INVALID_ARGUMENT, "x must be [channels][n]")
        n = x.shape[1]
        cap = self.next_out(n)
        out = np.empty((self.channels, cap), np.float32)
        got = C.c_size_t(0)
        check(load().earhip_src_process(self.h, C.c_size_t(n), _chan_ptrs(x), _chan_ptrs(out), C.c_size_t(cap), C.byref(got)))
        assert got.value == cap
        return out

    def process_device(self, nsamples, in_ptr, in_stride, out_ptr, out_stride, out_capacity):
        """planar float32 rows in device memory (e.g. torch tensors' data_ptr()); enqueues on the context's stream; returns the
        number of outputs written per row"""
        got = C.c_size_t(0)
        check(load().earhip_src_process_device(self.h, C.c_size_t(nsamples), C.c_void_p(in_ptr), C.c_size_t(in_stride),
                                               C.c_void_p(out_ptr), C.c_size_t(out_stride), C.c_size_t(out_capacity), C.byref(got)))
        return got.value


# (S) delay matrix

class _DelaymixRoute(C.Structure):
    _fields_ = [("in_", C.c_int), ("out", C.c_int), ("delay", C.c_int), ("n_taps", C.c_int), ("taps", C.c_float * 32)]


class _DelaymixConfig(C.Structure):
    _fields_ = [("n_in", C.c_int), ("n_out", C.c_int), ("n_routes", C.c_int), ("routes", C.POINTER(_DelaymixRoute)),
                ("max_samples", C.c_size_t)]


class _DelaymixProperties(C.Structure):
    _fields_ = [("tile_out", C.c_int), ("launch_in", C.c_size_t), ("routes", C.c_int), ("history", C.c_int),
                ("max_fan_in", C.c_int), ("total_taps", C.c_int), ("device_bytes", C.c_size_t)]


def delaymix_fractional(delay, n_taps=16, beta=8.0):
    """(whole, taps float64 [n_taps]): a delay of `delay` samples as a route's whole delay and taps; n_taps = 1 rounds to the
    nearest sample, an even n_taps is a Kaiser-windowed sinc centred on the fraction with unit DC gain.  A pure host function"""
    T = _src_int("n_taps", n_taps)
    whole, taps = C.c_int(0), np.zeros(T if 0 < T <= 32 else 1, np.float64)
    load().earhip_delaymix_fractional.argtypes = [C.c_double, C.c_int, C.c_double, C.c_void_p, C.c_void_p]
    check(load().earhip_delaymix_fractional(float(delay), T, float(beta), C.byref(whole), C.c_void_p(taps.ctypes.data)))
    return whole.value, taps


def delaymix_align(distances_m, sample_rate, speed_of_sound=343.0):
    """(delay_samples, gain), float64 [n]: loudspeakers at distances_m brought to the farthest one's arrival time and level.
    A pure host function"""
    d = np.ascontiguousarray(np.asarray(distances_m, np.float64).reshape(-1))
    delay, gain = np.zeros(max(d.size, 1), np.float64), np.zeros(max(d.size, 1), np.float64)
    load().earhip_delaymix_align.argtypes = [C.c_int, C.c_void_p, C.c_double, C.c_double, C.c_void_p, C.c_void_p]
    check(load().earhip_delaymix_align(d.size, C.c_void_p(d.ctypes.data) if d.size else None, float(sample_rate),
                                       float(speed_of_sound), C.c_void_p(delay.ctypes.data), C.c_void_p(gain.ctypes.data)))
    return delay[:d.size], gain[:d.size]


class DelayMatrix(_BusStage):
    """(S) a sparse matrix of delayed short FIRs: routes = [(in, out, delay, taps)], delay a whole number of samples in
    [0, 65536], taps 1 .. 32 float32 values (a gain: one tap); out_k[n] = the fmaf chain over the routes into k in list order of
    taps[j] * x_in[n - delay - j]; the same bits however the stream is cut into calls."""
    _stem = "delaymix"

    def __init__(self, ctx, n_in, n_out, routes, max_samples=48000):
        n_in, n_out = _src_int("n_in", n_in), _src_int("n_out", n_out)
        if isinstance(max_samples, bool) or not isinstance(max_samples, (int, np.integer)) or int(max_samples) < 1:
            raise InvalidArgument(INVALID_ARGUMENT, "max_samples must be an integer >= 1")
        routes = list(routes)
        arr = (_DelaymixRoute * max(len(routes), 1))()
        for i, route in enumerate(routes):
            if len(route) != 4:
                raise InvalidArgument(INVALID_ARGUMENT, "a route is (in, out, delay, taps)")
            rin, rout, delay, taps = route
            h = np.asarray(taps, np.float64).reshape(-1)
            with np.errstate(over="ignore"):
                h = h.astype(np.float32)
            arr[i].in_, arr[i].out, arr[i].delay = _src_int("a route's in", rin), _src_int("a route's out", rout), _src_int("a route's delay", delay)
            arr[i].n_taps = h.size
            for j in range(min(h.size, 32)):
                arr[i].taps[j] = h[j]
        self.ctx, self.n_in, self.n_out = ctx, n_in, n_out
        self.max_samples = int(max_samples)
        cfg = _DelaymixConfig(n_in, n_out, len(routes), arr, self.max_samples)
        self.h = C.c_void_p()
        check(load().earhip_delaymix_create(ctx.h if ctx is not None else None, C.byref(cfg), C.byref(self.h)))

    def info(self):
        """dict: tile_out, launch_in, routes, history (H), max_fan_in, total_taps, device_bytes"""
        v = _DelaymixProperties()
        check(load().earhip_delaymix_info(self.h, C.byref(v)))
        return {name: getattr(v, name) for name, _ in _DelaymixProperties._fields_}

    def process(self, x):
        """x [n_in][n] host array, any n -> [n_out][n]"""
        x = _f32(x)
        if x.ndim != 2 or x.shape[0] != self.n_in:
            raise InvalidArgument(INVALID_ARGUMENT, "x must be [n_in][n]")
        n = x.shape[1]
        out = np.empty((self.n_out, n), np.float32)
        check(load().earhip_delaymix_process(self.h, C.c_size_t(n), _chan_ptrs(x), _chan_ptrs(out)))
        return out

    def process_device(self, nsamples, in_ptr, in_stride, out_ptr, out_stride):
        """planar float32 rows in device memory (e.g. torch tensors' data_ptr()); enqueues on the context's stream"""
        check(load().earhip_delaymix_process_device(self.h, C.c_size_t(nsamples), C.c_void_p(in_ptr), C.c_size_t(in_stride),
                                                    C.c_void_p(out_ptr), C.c_size_t(out_stride)))
