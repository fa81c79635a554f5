"""Using a trained flow (include/realnvp_hip.h, "latents"): encode images to
latents, decode latents, sample at a temperature, interpolate.

``FlowCodec`` is built like ``FlowScorer``: eval mode, one ``FlowProgram``
(walked forwards to encode, backwards to decode), the weight-norm refresh
once per public call.  One captured graph is one batch of one direction:

  encode   rnvp_score_in_fwd (the logit transform) + the forward program
  decode   the inverse program + rnvp_latent_out
  sample   rnvp_latent_draw + the inverse program + rnvp_latent_out

and is replayed for every batch of every later call.  What changes between
replays (the destination, the running global index, the number of valid rows,
the temperature) lives in a device-resident ``rnvp_latent_ctl`` block that the
kernels advance themselves and the host only writes with stream-ordered
copies: no re-capture for a ragged last batch, another N or another
temperature, and no host synchronisation until the result is read.  (The
output format is a launch argument of rnvp_latent_out, so decode and sample
keep one graph per format actually asked for; the Philox-noise encode is a
second encode graph, the explicit-noise one serves "mid" and a tensor.)

A sample belongs to its index: image i of ``sample(n, first=f)`` is a function
of (seed, f + i, temperature, weights) alone -- the same image at any batch
size and in any later call, which is what a fixed progression over the epochs
of a training run needs (the reference's
samples/realnvp_celeba_fixed_progression.jpg).

The host mirrors at the end (float64 numpy, no GPU) document the draw and the
mix; the tests compare the kernels against them.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from .engine import stream_ptr, upload, weights_key, wn_forward, wn_table
from .program import FlowProgram, capture_graph, current_wn_table

U8_MODES = {None: _lib.RNVP_OUT_F32, "round": _lib.RNVP_OUT_U8_ROUND, "floor": _lib.RNVP_OUT_U8_FLOOR}
MIX_MODES = {"lerp": _lib.RNVP_MIX_LERP, "slerp": _lib.RNVP_MIX_SLERP}


def check_u8(u8):
    """the output format: None (fp32), "round" (save_image's rule) or "floor"
    (the inverse of the dequantisation)"""
    if u8 is not None and not (isinstance(u8, str) and u8 in U8_MODES):
        raise ValueError('u8 must be None, "round" or "floor", got %r' % (u8,))
    return U8_MODES[u8]


def check_temperature(t):
    if isinstance(t, bool) or not isinstance(t, (int, float)) or not (t >= 0) or t == float("inf"):
        raise ValueError("temperature must be a finite number >= 0, got %r" % (t,))
    return float(t)


def _check_count(name, v, least):
    if isinstance(v, bool) or not isinstance(v, int) or v < least:
        raise ValueError("%s must be an int >= %d, got %r" % (name, least, v))
    return v


class FlowCodec:
    def __init__(self, model, batch_size, dtype=None, constraint=0.9, seed=0, temperature=1.0, graph=True):
        _check_count("batch_size", batch_size, 1)
        self.temperature = check_temperature(temperature)
        self.dev = next(model.parameters()).device
        if self.dev.type != "cuda":
            raise RuntimeError("FlowCodec needs the model on a HIP device")
        if model.training:
            raise RuntimeError("FlowCodec works in eval mode (train.py:253-259 runs after model.eval())")
        self.model = model
        self.B = batch_size
        self.dtype = dtype or next(model.couplings()).compute_dtype
        self.constraint, self.seed = constraint, seed
        Cc, S = model.channels, model.image_size
        self.shape = (Cc, S, S)
        self.D = Cc * S * S
        f32 = dict(device=self.dev, dtype=torch.float32)
        self.pix = torch.zeros(batch_size, Cc, S, S, **f32)
        self.noise = torch.full((batch_size, Cc, S, S), 0.5, **f32)
        self._noise_is_mid = True
        # [0]: rnvp_score_in_fwd adds the transform's log-det, [1]: the couplings theirs; an encode has no use
        # for either, so they are neither read nor zeroed (the graph holds library launches only)
        self.acc = torch.zeros(2, batch_size, **f32)
        # encode: a private scoring block, one draw per image; only `first` (the image's index, which keys
        # the Philox noise) ever changes
        self.enc_ctl = upload(bytes(_lib.ScoreCtl(None, 0, 0, 0, 0.0, batch_size, 1, 0, 0)), self.dev)
        self.ctl_buf = upload(bytes(_lib.LatentCtl(None, 0, 0, 0, self.temperature, batch_size, 0, 0)), self.dev)
        self._n_valid = batch_size      # what the latent block's n_valid holds
        self.program = FlowProgram(model, batch_size, self.dev, self.dtype, False)
        self.x, self.z = self.program.x, self.program.z
        self.engines = list(dict.fromkeys(st.eng for st in self.program.couplings))
        self.table = wn_table(self.engines, self.dtype, self.dev)
        self._wkey = weights_key(self.engines, self.dtype)
        self.graphs = {}                # (kind, variant) -> captured graph, built on first use
        self.use_graph = graph

    # ------------------------------------------------------------- plumbing
    def _refresh(self):
        """Start of every public call: the weight-norm table follows
        parameters that moved (graphs captured with the old one are dropped),
        the packed weights follow their values (a FlowTrainer step, the
        averaged weights inside ema_weights())."""
        self.table, self._wkey, moved = current_wn_table(self.engines, self.dtype, self.dev, self._wkey, self.table)
        if moved:
            self.graphs = {}
        if self.table is not None:
            wn_forward(self.table, self.dtype)

    @staticmethod
    def _field_of(buf, struct, name):
        f = getattr(struct, name)
        dt = {C.c_int: torch.int32, C.c_longlong: torch.int64, C.c_float: torch.float32}[dict(struct._fields_)[name]]
        return buf[f.offset:f.offset + f.size].view(dt)

    def _field(self, name):
        """a one-element tensor view of a field of the latent block"""
        return self._field_of(self.ctl_buf, _lib.LatentCtl, name)

    def _begin_out(self, n, u8, first=0, temperature=None):
        """A fresh destination of n rows and the block pointing at it with
        row 0 = global index `first` (the block addresses rows by their global
        index, so its dst is `first` rows in front of the tensor and its
        capacity first + n: the rows before `first` are never addressed)."""
        out = torch.empty((n,) + self.shape, device=self.dev, dtype=torch.float32 if u8 is None else torch.uint8)
        T = self.temperature if temperature is None else temperature
        dst = (out.data_ptr() - first * self.D * out.element_size()) & 0xFFFFFFFFFFFFFFFF
        blk = _lib.LatentCtl(dst, first + n, first, 0, T, self.B, 0, 0)
        self.ctl_buf.copy_(upload(bytes(blk), self.dev))
        self._n_valid = self.B
        return out

    def _set_rows(self, rows):
        if rows != self._n_valid:
            self._field("n_valid").fill_(rows)
            self._n_valid = rows

    def _run(self, key, run, restore=()):
        """one batch: replay the graph of `key` (captured on first use) or launch eagerly"""
        if not self.use_graph:
            run()
            return
        g = self.graphs.get(key)
        if g is None:
            # capture_graph runs the batch for real before it records one: blocks the run advances go back
            snaps = [(b, b.clone()) for b in restore]
            g = self.graphs[key] = capture_graph(run)
            for b, s in snaps:
                b.copy_(s)
        g.replay()

    def _forward(self, noise):
        L = _lib.lib()
        L.score_in_fwd(self.pix.data_ptr(), noise.data_ptr() if noise is not None else None, self.seed,
                       self.enc_ctl.data_ptr(), float(self.constraint), self.x.data_ptr(), self.acc[0].data_ptr(),
                       *self.pix.shape, stream_ptr())
        self.program.forward(lambda k, st: st.eng.forward(st.x, False, self.dtype, False, saved=st.saved,
                                                          prepare=False, ldj_sample=self.acc[1], z_out=st.z))

    def _inverse(self, mode, draw):
        L = _lib.lib()
        s = stream_ptr()
        ctl = self.ctl_buf.data_ptr()
        if draw:
            L.latent_draw(self.z.data_ptr(), self.seed, ctl, self.B, self.D, s)
        self.program.inverse(lambda k, st: st.eng.reverse(st.z, False, self.dtype, saved=st.saved, out=st.x,
                                                          want_ldj=False, prepare=False))
        L.latent_out(self.x.data_ptr(), ctl, float(self.constraint), self.B, self.D, mode, s)

    def _images(self, t, what):
        if not isinstance(t, torch.Tensor) or t.dim() != 4 or tuple(t.shape[1:]) != self.shape:
            raise ValueError("FlowCodec %s is [N, %d, %d, %d], got %s"
                             % ((what,) + self.shape + (tuple(getattr(t, "shape", ())) or type(t).__name__,)))
        return t

    # --------------------------------------------------------------- public
    def set_temperature(self, temperature):
        """The prior's standard deviation for the following samples: a
        stream-ordered write into the block, the captured graphs stay."""
        self.temperature = check_temperature(temperature)
        self._field("temperature").fill_(self.temperature)

    def encode(self, batches, noise="mid"):
        """fp32 device tensor [N, C, S, S]: the latents of N images in [0, 1].
        batches: one tensor [N, C, S, S], or an iterable of pixel batches (or
        (pixels, target) pairs) of at most B rows, the last one ragged, e.g.
        data.DeviceLoader(valid_set, B, dev, shuffle=False).
        noise: "mid" (u = 0.5, the deterministic encoding), "philox" (keyed by
        the image's index in the pass, like FlowScorer's) or a tensor
        [N, C, S, S] of values in [0, 1)."""
        def pixels(b):
            return b[0] if isinstance(b, (tuple, list)) else b
        explicit = isinstance(noise, torch.Tensor)
        if not explicit and not (isinstance(noise, str) and noise in ("mid", "philox")):
            raise ValueError('noise must be "mid", "philox" or a tensor, got %r' % (noise,))

        def checked(b):
            b = pixels(b)
            if not (1 <= self._images(b, "batch").shape[0] <= self.B):
                raise ValueError("FlowCodec batch is 1..%d rows, got %d" % (self.B, b.shape[0]))
            return b
        loader = getattr(batches, "loader", batches)
        if isinstance(batches, torch.Tensor):
            N = self._images(batches, "images").shape[0]
            batches = [batches[i:i + self.B] for i in range(0, N, self.B)]
        elif hasattr(loader, "dataset"):
            N = len(loader.dataset)             # batches are checked as they arrive
        else:
            batches = [checked(b) for b in batches]
            N = sum(int(b.shape[0]) for b in batches)
        if explicit and tuple(noise.shape) != (N,) + self.shape:
            raise ValueError("FlowCodec noise is %s, got %s" % ((N,) + self.shape, tuple(noise.shape)))
        self._refresh()
        out = torch.empty((N,) + self.shape, device=self.dev, dtype=torch.float32)
        first = self._field_of(self.enc_ctl, _lib.ScoreCtl, "first")
        with torch.no_grad():
            if noise == "mid" and not self._noise_is_mid:
                self.noise.fill_(0.5)
                self._noise_is_mid = True
            i = 0
            for b in batches:
                b = checked(b)
                rows = b.shape[0]
                if i + rows > N:
                    raise RuntimeError("FlowCodec.encode: more than the %d images the loader announced" % N)
                self.pix[:rows].copy_(b)
                if rows < self.B:
                    self.pix[rows:].zero_()          # padding rows: zeros in, nothing out
                if explicit:
                    self.noise[:rows].copy_(noise[i:i + rows])
                    self._noise_is_mid = False
                elif noise == "philox":
                    first.fill_(i)
                if noise == "philox":
                    self._run(("encode", "philox"), lambda: self._forward(None))
                else:
                    self._run(("encode", "noise"), lambda: self._forward(self.noise))
                out[i:i + rows].copy_(self.z[:rows])
                i += rows
        return out[:i]

    def _decode(self, z, mode, u8):
        N = z.shape[0]
        out = self._begin_out(N, u8)
        with torch.no_grad():
            for i in range(0, N, self.B):
                rows = min(self.B, N - i)
                self.z[:rows].copy_(z[i:i + rows])
                if rows < self.B:
                    self.z[rows:].zero_()
                self._set_rows(rows)
                self._run(("decode", mode), lambda: self._inverse(mode, False), restore=(self.ctl_buf,))
        return out

    def decode(self, z, u8=None):
        """[N, C, S, S] images of the latents z [N, C, S, S]: fp32 (the value
        FlowSampler returns, unclamped), or uint8 with u8 = "round"
        (torchvision's save_image rule) or "floor" (the exact inverse of the
        dequantisation: decode(encode(x, "mid"), u8="floor") is x's bytes)."""
        mode = check_u8(u8)
        self._images(z, "latents")
        self._refresh()
        return self._decode(z, mode, u8)

    def sample(self, n, first=0, temperature=None, u8=None):
        """n images drawn from the prior at the block's temperature (or this
        call's): image i is sample first + i of the seed's stream."""
        _check_count("n", n, 1)
        _check_count("first", first, 0)
        mode = check_u8(u8)
        T = None if temperature is None else check_temperature(temperature)
        self._refresh()
        out = self._begin_out(n, u8, first, T)
        with torch.no_grad():
            for i in range(0, n, self.B):
                self._set_rows(min(self.B, n - i))
                self._run(("sample", mode), lambda: self._inverse(mode, True), restore=(self.ctl_buf,))
            if T is not None and T != self.temperature:
                self._field("temperature").fill_(self.temperature)
        return out

    def interpolate(self, pix_a, pix_b, steps=8, mode="slerp", u8=None):
        """[P, steps, C, S, S]: the images along the path between the "mid"
        latents of pix_a[p] and pix_b[p] at t = linspace(0, 1, steps), mode
        "slerp" (spherical) or "lerp"."""
        _check_count("steps", steps, 2)
        if not (isinstance(mode, str) and mode in MIX_MODES):
            raise ValueError('mode must be "slerp" or "lerp", got %r' % (mode,))
        out_mode = check_u8(u8)
        self._images(pix_a, "pix_a")
        self._images(pix_b, "pix_b")
        if pix_a.shape[0] != pix_b.shape[0] or pix_a.shape[0] < 1:
            raise ValueError("FlowCodec.interpolate needs as many images in pix_a as in pix_b (>= 1), got %d and %d"
                             % (pix_a.shape[0], pix_b.shape[0]))
        P = pix_a.shape[0]
        za, zb = self.encode(pix_a, "mid"), self.encode(pix_b, "mid")
        t = torch.linspace(0.0, 1.0, steps, device=self.dev, dtype=torch.float32)
        lat = torch.empty((P, steps) + self.shape, device=self.dev, dtype=torch.float32)
        ws = torch.empty(3 * P, device=self.dev, dtype=torch.float64)
        _lib.lib().latent_mix(za.data_ptr(), zb.data_ptr(), t.data_ptr(), lat.data_ptr(), P, steps, self.D,
                              MIX_MODES[mode], ws.data_ptr(), stream_ptr())
        out = self._decode(lat.view((P * steps,) + self.shape), out_mode, u8)
        return out.view((P, steps) + self.shape)


# ---------------------------------------------------------------------------
# host mirrors (float64 numpy, no GPU)
# ---------------------------------------------------------------------------
PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85
_M32 = np.uint64(0xFFFFFFFF)


def philox4x32(counter_words, key_words):
    """Philox4x32-10 (Salmon et al. 2011).  counter_words: [..., 4] 32-bit
    words, key_words: [2] (or [..., 2]); returns the [..., 4] output words as
    uint32.  The device generator (csrc/latent.hip; csrc/flow_ops.hip keeps
    the first word) uses counter (index low, index high, 0, 0) and key
    (seed low, seed high)."""
    c = np.asarray(counter_words, dtype=np.uint64) & _M32
    k = np.asarray(key_words, dtype=np.uint64) & _M32
    c0, c1, c2, c3 = (c[..., j].copy() for j in range(4))
    k0, k1 = k[..., 0].copy(), k[..., 1].copy()
    for _ in range(10):
        p0 = np.uint64(PHILOX_M0) * c0          # 32 x 32 -> 64 bits: no wrap
        p1 = np.uint64(PHILOX_M1) * c2
        n0 = (p1 >> np.uint64(32)) ^ c1 ^ k0
        n2 = (p0 >> np.uint64(32)) ^ c3 ^ k1
        c1, c3, c0, c2 = p1 & _M32, p0 & _M32, n0, n2
        k0 = (k0 + np.uint64(PHILOX_W0)) & _M32
        k1 = (k1 + np.uint64(PHILOX_W1)) & _M32
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def prior_reference(seed, first, rows, n, temperature=1.0):
    """float64 [rows, n]: what rnvp_latent_draw writes for rows of n elements
    starting at global row `first`.  Element e of global row r has the counter
    (i & 0xffffffff, i >> 32, 0, 0) with i = r * n + e (mod 2^64); of the
    output words, u1 = ((w0 >> 8) + 1) 2^-24 in (0, 1], u2 = (w1 >> 8) 2^-24 in
    [0, 1), g = sqrt(-2 ln u1) cos(2 pi u2); the value is temperature (rounded
    to fp32, as the block holds it) times g."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    base = (int(first) * int(n)) & 0xFFFFFFFFFFFFFFFF
    i = np.uint64(base) + np.arange(int(rows) * int(n), dtype=np.uint64)      # wraps like the device's uint64
    ctr = np.stack([i & _M32, i >> np.uint64(32), np.zeros_like(i), np.zeros_like(i)], axis=-1)
    w = philox4x32(ctr, np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64))
    u1 = ((w[:, 0] >> 8).astype(np.float64) + 1.0) * 2.0 ** -24
    u2 = (w[:, 1] >> 8).astype(np.float64) * 2.0 ** -24
    g = np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)
    return (float(np.float32(temperature)) * g).reshape(int(rows), int(n))


def mix_reference(a, b, t, mode="slerp"):
    """float64 [P, T, ...]: rnvp_latent_mix of the endpoint latents a, b
    [P, ...] at the steps t [T].  "lerp": (1 - t) a + t b.  "slerp": with
    c = clamp(a.b / (|a| |b|), -1, 1) per pair, the lerp weights when
    1 - |c| < 1e-9 or a norm is zero, else Om = acos(c) and
    sin((1 - t) Om) / sin Om, sin(t Om) / sin Om."""
    if mode not in MIX_MODES:
        raise ValueError('mode must be "slerp" or "lerp", got %r' % (mode,))
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    t = np.asarray(t, dtype=np.float64).reshape(-1)
    if a.shape != b.shape or a.ndim < 2:
        raise ValueError("mix_reference endpoints are two [P, ...] arrays of one shape, got %s and %s"
                         % (a.shape, b.shape))
    P = a.shape[0]
    fa, fb = a.reshape(P, -1), b.reshape(P, -1)
    wa = np.broadcast_to(1.0 - t, (P, t.size)).copy()
    wb = np.broadcast_to(t, (P, t.size)).copy()
    if mode == "slerp":
        for p in range(P):
            na, nb = np.sqrt(fa[p] @ fa[p]), np.sqrt(fb[p] @ fb[p])
            if not (na > 0.0 and nb > 0.0):
                continue
            c = min(max((fa[p] @ fb[p]) / (na * nb), -1.0), 1.0)
            if 1.0 - abs(c) < 1e-9:
                continue
            om = np.arccos(c)
            wa[p], wb[p] = np.sin((1.0 - t) * om) / np.sin(om), np.sin(t * om) / np.sin(om)
    out = wa[:, :, None] * fa[:, None, :] + wb[:, :, None] * fb[:, None, :]
    return out.reshape((P, t.size) + a.shape[1:])
