"""``IntraNoAR`` -- the I-frame codec behind the reference's API
(/root/reference/DCVC_HEM/src/models/image_model.py:16-200), on the same HIP kernels.

    IntraNoAR(N=192, anchor_num=4)
    .forward(x, q_scale) -> {x_hat, mse, bit, bpp, bpp_y, bpp_z}           :54-106
    .compress(x, q_scale) -> {"bit_stream"}  (+ "x_hat")                   :148-177
    .decompress(bit_stream, height, width, q_scale) -> {"x_hat"}           :179-200
    .encode_decode(x, q_scale, output_path=None, pic_width=None, pic_height=None)  :114-146
"""
from __future__ import annotations

import time

import torch

from . import stream as S
from .dmc import CodecBase, _load_upstream, _param_grads, _qgrad
from .params import intra_spec


class _IntraFn(torch.autograd.Function):
    """One I picture in training mode as a single autograd node (the counterpart of dmc._FrameFn): forward records a
    grad.Tape on the HIP engine, backward replays it with the kernels of include/dcvc_hip_grad.h.  Inputs after the
    q-scale are the model's parameters; outputs are the per-sample sums (bits_y, bits_z, squared error) and x_hat."""

    @staticmethod
    def forward(ctx, model, x, q, *params):
        from .grad import Tape

        ctx.set_materialize_grads(False)
        tape = Tape(model.engine())
        o, sums = model._train_frame(tape, x.detach(), q.detach())
        ctx.tape, ctx.params, ctx.q_shape, ctx.out_view = tape, params, q.shape, o["x_hat"]
        return sums["bits_y"], sums["bits_z"], sums["sq"], o["x_hat"].nchw()

    @staticmethod
    def backward(ctx, g_y, g_z, g_sq, g_xhat):
        tape = ctx.tape
        if tape is None:
            raise RuntimeError("this picture's tape was already consumed (retain_graph is not supported)")
        e = tape.e
        _load_upstream(tape, (("bits_y", g_y), ("bits_z", g_z), ("sq", g_sq)))
        if g_xhat is not None:  # a loss computed on the reconstruction by the caller (perceptual terms)
            e.from_nchw(g_xhat, tape.grad(ctx.out_view))
        tape.backward()
        grads = _param_grads(ctx.params, ctx.needs_input_grad[3:], lambda p: tape.pgrads.get(id(p)))
        gq = _qgrad(tape.q["y"]["dq_scale"], ctx.q_shape, ctx.needs_input_grad[2])
        ctx.tape = None
        return (None, None, gq, *grads)


class IntraNoAR(CodecBase):
    _tag = "intra"
    _distribution = "gaussian"
    _z_names = ("bit_estimator_z",)

    def __init__(self, N=192, anchor_num=4, seed=0, precision=None):
        super().__init__(intra_spec(N, anchor_num), seed=seed, precision=precision)
        self.N = int(N)
        self.anchor_num = int(anchor_num)

    @staticmethod
    def get_q_scales_from_ckpt(ckpt_path):
        return S.get_state_dict(ckpt_path)["q_scale"].reshape(-1)

    def _synthesis(self, net, y_hat, N, H, W, clamp):
        d = net.decoder_stack("dec", y_hat)
        u = net.unet("refine.0", d)
        k = self._out_set() if self.engine().tape is None else 0  # (a recorded forward owns fresh buffers)
        x_hat = net.buf(f"dpb{k}.x_hat", N=N, H=H, W=W, C=3)
        net.conv("refine.1", u, out=x_hat, out_slope="clamp01" if clamp else None)
        return x_hat

    def get_curr_q(self, q_scale):
        """image_model.py:50-52: max(q_basic, 0.5) * q_scale."""
        return torch.clamp_min(self.P("q_basic"), 0.5) * q_scale

    def _run(self, x, q_scale, mode, tape=None, q_map=None):
        """mode 'estimate' / 'compress' / 'train' (a recorded forward: straight-through rounding, y_res kept).
        q_map: see compress()."""
        e = self.engine()
        net = self._net
        Nb, _, H, W = x.shape
        assert H % 64 == 0 and W % 64 == 0, "pad to a multiple of 64 first (stream.get_padding_size)"
        q_map = self._qmap(q_map, Nb, H, W)
        q = self._qvec(q_scale, Nb, "q_scale")
        qb = self.P("q_basic").reshape(-1)
        x3 = self._frame_in("x", x)
        if tape is not None:
            tape.mark_const(x3)  # the picture carries no gradient
        y_raw = net.encoder_stack("enc", x3)
        y = e.scale_channels(y_raw, net.buf("y", like=y_raw, C=self.N), qb, q, qkey="y", q_map=q_map)
        z = net.hyper_enc5("hyper_enc", y)
        z_hat = net.buf("z_hat", like=z, C=self.N)
        sym_z = e.ibuf("intra/sym_z", Nb * self.N * z.HW) if mode == "compress" else None
        self._wait_coder()
        e.round_symbols(z, z_hat, sym_z)
        fusion = net.three_convs("y_prior_fusion", net.hyper_dec("hyper_dec", z_hat))
        y_hat = net.buf("y_hat", like=y, C=self.N)
        r = self._dual_prior_encode("y", y, fusion, "y_spatial_prior", y_hat, qb, q, want_stats=(mode != "compress"),
                                    want_symbols=(mode == "compress"), want_res=(mode == "train"), qkey="y",
                                    q_map=q_map)
        x_hat = self._synthesis(net, y_hat, Nb, H, W, clamp=(mode == "compress"))  # compress == decoder output
        return dict(N=Nb, H=H, W=W, x3=x3, y=y, z=z, z_hat=z_hat, sym_z=sym_z, r=r, x_hat=x_hat, y_hat=y_hat)

    # ------------------------------------------------------------------ training-mode forward (round 4)
    def _train_frame(self, tape, x, q_scale):
        """Recorded forward of IntraNoAR.forward in training mode (image_model.py:54-100 with self.training: straight-through
        rounding, uniform noise on the residual and on z for the bit estimates, Gaussian likelihood).  The reference's
        trainers run the I-picture codec under no_grad (core/model/dcvc_hem.py:164-167), but its forward IS
        differentiable; this is that path.  Returns the views and the per-sample sums."""
        e = self.engine()
        e.tape = tape
        try:
            e.repack_all()
            N = x.shape[0]
            tape.qstate("y", self.P("q_basic"), self._qvec(q_scale, N, "q_scale"), N, self.N)
            o = self._run(x, tape.q["y"]["q_scale"], "train", tape=tape)
            sums = {}
            sums["sq"] = e.sq_err(o["x_hat"], o["x3"])
            tape.ops.append(("sq_err", "sq", o["x_hat"], o["x3"]))
            self._record_scale_bits(tape, sums, "bits_y", o["y"], o["r"], "y")
            self._record_factorized_bits(tape, sums, "bits_z", o["z"], "bit_estimator_z", "z")
            return o, sums
        finally:
            e.tape = None

    def _forward_train(self, x, q_scale):
        q = self.P("q_scale") if q_scale is None else q_scale
        q = q if torch.is_tensor(q) else torch.tensor(float(q), device=self.device)
        params = [p for n, p in self._pmap.items() if n != "q_scale"]
        bits_y, bits_z, sq, x_hat = _IntraFn.apply(self, x, q, *params)
        pix = x.shape[2] * x.shape[3]
        bpp_y, bpp_z = bits_y / pix, bits_z / pix
        res = {"x_hat": x_hat, "mse": sq / pix, "bit": (torch.sum(bpp_y + bpp_z) * pix).item(), "bpp": bpp_y + bpp_z,
               "bpp_y": bpp_y, "bpp_z": bpp_z}
        return self._ssim_keys(res, x, x_hat) if self.report_ssim else res

    def forward(self, x, q_scale=None):
        """Training mode (round 4): the differentiable forward of image_model.py:54-106 (`bit` stays a float, :102)."""
        if self.training:
            return self._forward_train(x, q_scale)
        with torch.no_grad():
            return self._forward_eval(x, q_scale)

    def _forward_eval(self, x, q_scale=None):
        e = self.engine()
        o = self._run(x, q_scale, "estimate")
        pix = o["H"] * o["W"]
        bpp_y = e.scale_bits(o["r"]["y_q"], o["r"]["scales_hat"], o["N"], o["y"].HW * self.N, gaussian=True) / pix
        bpp_z = e.factorized_bits(o["z_hat"], self._zblock("bit_estimator_z")) / pix
        mse = e.sq_err(o["x3"], o["x_hat"]) / pix
        res = {"x_hat": o["x_hat"].nchw(), "mse": mse, "bit": (torch.sum(bpp_y + bpp_z) * pix).item(),
               "bpp": bpp_y + bpp_z, "bpp_y": bpp_y, "bpp_z": bpp_z, "_views": o}
        return self._ssim_keys(res, x, res["x_hat"]) if self.report_ssim else res

    @torch.no_grad()
    def compress(self, x, q_scale, defer=False, coder="host", check_range=True, q_map=None, bit_map=False):
        """q_map: ROI-weighted quantisation (roi.q_map; CodecBase._qmap says what is taken): one factor per 16x16 cell on the
        quantisation step of y.  decompress() needs the same map.  None: exactly the launches and bytes without it.
        bit_map=True: the result also carries "bit_map", a bitmap.BitMap of the picture's z and y planes
        (CodecBase._bit_map).  False: exactly the launches, bytes and result keys without it."""
        if self.entropy_coder is None:
            raise RuntimeError("call update() before compress()/decompress()")
        o = self._run(x, q_scale, "compress", q_map=q_map)
        N = o["N"]  # N > 1: a batch of rate points (one q-scale per element), one independent stream each
        zs = o["z_hat"]
        planes = [  # image_model.py:168-171
            ("bit_estimator_z", o["sym_z"], None, (N, self.N, zs.H, zs.W)),
            ("scale", o["r"]["sym"][0], o["r"]["idx"][0], None),
            ("scale", o["r"]["sym"][1], o["r"]["idx"][1], None),
        ]
        bits = self._bit_map(bit_map, planes, N)
        pending = self._stage(planes, N, coder)
        return self._compress_result({"x_hat": o["x_hat"].nchw(), "_views": o}, pending, defer, check_range, bits)

    @torch.no_grad()
    def decompress(self, bit_stream, height, width, q_scale, coder=None, defer_check=False, check_range=True, q_map=None):
        """q_map: the map compress() was given (the stream does not carry it)."""
        return self._decompress_guarded(bit_stream, coder, defer_check, check_range, bit_stream, height, width, q_scale,
                                        q_map)

    def _decompress(self, bit_stream, height, width, q_scale, q_map=None):
        e = self.engine()
        net = self._net
        q = self._qvec(q_scale, 1, "q_scale")
        zh, zw = S.get_downsampled_shape(height, width, 64)
        q_map = self._qmap(q_map, 1, zh * 64, zw * 64)
        self._open_stream(bit_stream)
        sym = self._decode_factorized("bit_estimator_z", 1, self.N, zh, zw)
        z_hat = e.symbols_to_nhwc(sym, net.buf("z_hat", N=1, H=zh, W=zw, C=self.N))
        fusion = net.three_convs("y_prior_fusion", net.hyper_dec("hyper_dec", z_hat))
        y_hat = net.buf("y_hat", N=1, H=zh * 4, W=zw * 4, C=self.N)
        self._dual_prior_decode("y", fusion, "y_spatial_prior", y_hat, self.P("q_basic").reshape(-1), q, q_map=q_map)
        x_hat = self._synthesis(net, y_hat, 1, zh * 64, zw * 64, clamp=self._clamp_decoded)  # .clamp_(0, 1), :199
        self._close_stream()
        return {"x_hat": x_hat.nchw()}

    def encode_decode(self, x, q_scale, output_path=None, pic_width=None, pic_height=None):
        if output_path is None:
            return self.forward(x, q_scale)
        assert pic_height is not None and pic_width is not None
        t0 = time.time()
        q_scale, q_index = S.get_rounded_q(q_scale)
        compressed = self.compress(x, q_scale)
        S.encode_i(pic_height, pic_width, q_index, compressed["bit_stream"], output_path)
        bit = S.filesize(output_path) * 8
        t1 = time.time()
        height, width, q_index, bit_stream = S.decode_i(output_path)
        decompressed = self.decompress(bit_stream, height, width, q_index / 100, coder="host")
        torch.cuda.synchronize(self.device)
        t2 = time.time()
        return {"bit": bit, "x_hat": decompressed["x_hat"], "encoding_time": t1 - t0, "decoding_time": t2 - t1}
