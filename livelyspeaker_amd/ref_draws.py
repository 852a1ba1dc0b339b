"""Every normal (and the one Philox key) the drop-in draws on behalf of the reference: the single statement of the "identical seeds"
draw order.  ``gaussian_diffusion.py`` and ``long_form.py`` draw nothing themselves; they ask a ``RefDraws``
bound to one torch generator -- the CPU's (``noise_source='torch_cpu'``) or the model's GPU's (``'torch_device'``) -- so
``torch.manual_seed(s)`` fixes every draw of a call in the reference's order, shapes and memory orders.

``th.randn`` / ``th.randn_like`` are looked up through the torch module at call time: a caller (or test) that replaces them wants to
see every draw, and ``intercepted()`` is how the native streams learn that they must stand aside.
"""
from __future__ import annotations

import numpy as np
import torch as th

from . import _lib, torch_rng


def intercepted() -> bool:
    """Has somebody replaced torch's draw functions since gaussian_diffusion was imported?"""
    from . import gaussian_diffusion as gd
    return th.randn is not gd._TH_RANDN or th.randn_like is not gd._TH_RANDN_LIKE


def host_native(diffusion, draws_between=False, first_contiguous=True) -> int:
    """May the host draws of this call be made natively from torch's CPU generator state (torch_rng.py: mt19937 + torch's two normal
    transforms restated in C++) -- the variant that reproduces this torch build bit for bit, or -1.  Only when the loop draws nothing
    else in between (inpainting re-noise draws), its first x is contiguous and nobody has replaced torch's draw functions."""
    ok = diffusion.native_host_rng and not draws_between and first_contiguous and not intercepted()
    native = torch_rng.variant() if ok else -1
    diffusion.last_host_rng_native = native >= 0
    return native


def philox_key() -> int:
    """One 62-bit key from torch's CPU generator (torch.manual_seed reproduces a philox-mode run)."""
    return int(th.randint(0, 2 ** 62, (1,)).item())


class RefDraws:
    """The reference's draws from torch's generator of ``rdev``."""

    def __init__(self, rdev):
        self.rdev = th.device(rdev)

    def _proto(self, t, shape):
        """The prototype of a randn_like: the caller's tensor where the reference draws like it (strides and all), else contiguous."""
        if not th.is_tensor(t):
            return th.empty(shape, device=self.rdev)
        return t.detach().cpu() if self.rdev.type == "cpu" else t

    def x_T(self, shape, const_noise=False):
        """The loops' start, th.randn(*shape) (gaussian_diffusion.py:701-704); const_noise repeats the first row."""
        x = th.randn(*shape, device=self.rdev)
        return x[[0]].repeat(shape[0], 1, 1, 1) if const_noise else x

    def like(self, x, dtype=th.float32):
        """randn_like(x): follows x's strides, i.e. consumes the generator in x's memory order (:252, :318, :543, :787, :1617)."""
        return th.randn_like(x, device=self.rdev, dtype=dtype)

    def pair(self, B, D):
        """The style eps of one model evaluation, [B, 1, D] each: ClassifierFreeSampleModel runs the cond pass, then the uncond pass,
        and each reparameterizes once (RAG.py:10-13)."""
        eps_c = th.randn(B, 1, D, device=self.rdev)
        return eps_c, th.randn(B, 1, D, device=self.rdev)

    def pair_into(self, row):
        """The same pair into one [2, B, D] tape row."""
        eps_c, eps_u = self.pair(row.shape[1], row.shape[2])
        row[0], row[1] = eps_c[:, 0], eps_u[:, 0]

    def plms_tape(self, n_eval, B, D):
        """plms_sample_loop's draws after x_T: one pair per model evaluation, no step noise (:1016-1098)."""
        eps = th.empty(n_eval, 2, B, D, device=self.rdev)
        for e in range(n_eval):
            self.pair_into(eps[e])
        return eps

    def steps(self, shape, D, n_exec, first=None, inpainted=None, diffusion=None):
        return _Steps(self, shape, D, n_exec, first, inpainted, diffusion)

    def windows(self, diffusion, W, n_exec, shape, D, batches=None):
        """Long-form: W calls of the sample loop, window after window -- x_T, then that window's steps (contiguous first x).

        ``batches`` (one batch size per window; ``shape[0]`` is then ignored): window w is a call at batch ``batches[w]``, and the
        tapes come back packed -- x [sum batches, J, F, T], and flat eps / noise holding per window [n_exec, 2, B_w, D] /
        [n_exec, B_w, J, F, T], concatenated.  What W single-window calls at those batches draw one after the other."""
        if batches is None:
            steps = self.steps(shape, D, n_exec, diffusion=diffusion)
            x, eps, nz = th.empty((W,) + shape), th.empty(W, n_exec, 2, shape[0], D), th.empty((W, n_exec) + shape)
            for w in range(W):
                x[w] = self.x_T(shape)
                steps.run(0, eps[w], nz[w])
            return x, eps, nz
        batches = [int(b) for b in batches]
        if len(batches) != W or min(batches) < 1:
            raise ValueError(f"batches must hold {W} batch sizes >= 1, got {batches}")
        rest, total = tuple(shape[1:]), sum(batches)
        per_x = int(np.prod(rest))
        x, eps, nz = th.empty((total,) + rest), th.empty(total * n_exec * 2 * D), th.empty(total * n_exec * per_x)
        first = 0
        for Bw in batches:
            wshape = (Bw,) + rest
            x[first:first + Bw] = self.x_T(wshape)
            self.steps(wshape, D, n_exec, diffusion=diffusion).run(
                0, eps[first * n_exec * 2 * D:(first + Bw) * n_exec * 2 * D].view(n_exec, 2, Bw, D),
                nz[first * n_exec * per_x:(first + Bw) * n_exec * per_x].view((n_exec,) + wshape))
            first += Bw
        return x, eps, nz

    def edit_windows(self, diffusion, n_run, n_exec, shape, D, noised, batches=None):
        """Timeline edit (long_form.edit_long): what one public sampling call per window that runs draws, one after the other -- x_T,
        then that window's steps with the inpainting branch's re-noise draw between the model call and the step noise when ``noised``
        (the TED tree; its prototype is the window's slice of the timeline, contiguous).  Returns (x [n_run, B, J, F, T], eps
        [n_run, n_exec, 2, B, D], noise [n_run, n_exec, B, J, F, T], re-noise of the same shape or None).

        ``batches`` (one batch size per window that runs; ``shape[0]`` is then ignored): the compact edit -- window i is a call at
        batch ``batches[i]``, and the tapes come back packed as in ``windows(batches=)``: x [sum batches, J, F, T], and flat eps /
        noise / re-noise holding per window [n_exec, 2, A_i, D] / [n_exec, A_i, J, F, T], concatenated."""
        shape = tuple(shape)
        if batches is not None:
            batches = [int(b) for b in batches]
            if len(batches) != n_run or min(batches) < 1:
                raise ValueError(f"batches must hold {n_run} batch sizes >= 1, got {batches}")
            rest, total = shape[1:], sum(batches)
            per_x = int(np.prod(rest))
            x, eps, nz = th.empty((total,) + rest), th.empty(total * n_exec * 2 * D), th.empty(total * n_exec * per_x)
            inz = th.zeros(total * n_exec * per_x) if noised else None
            first = 0
            for A in batches:
                wshape = (A,) + rest
                x[first:first + A] = self.x_T(wshape)
                steps = self.steps(wshape, D, n_exec, inpainted=th.empty(wshape, device=self.rdev) if noised else None, diffusion=diffusion)
                steps.run(0, eps[first * n_exec * 2 * D:(first + A) * n_exec * 2 * D].view(n_exec, 2, A, D),
                          nz[first * n_exec * per_x:(first + A) * n_exec * per_x].view((n_exec,) + wshape))
                if noised:
                    inz[first * n_exec * per_x:(first + A) * n_exec * per_x].view((n_exec,) + wshape).copy_(steps.inz)
                first += A
            return x, eps, nz, inz
        x, eps, nz = th.empty((n_run,) + shape), th.empty(n_run, n_exec, 2, shape[0], D), th.empty((n_run, n_exec) + shape)
        inz = th.zeros((n_run, n_exec) + shape) if noised else None
        proto = th.empty(shape, device=self.rdev) if noised else None
        for i in range(n_run):
            x[i] = self.x_T(shape)
            steps = self.steps(shape, D, n_exec, inpainted=proto, diffusion=diffusion)
            steps.run(0, eps[i], nz[i])
            if noised:
                inz[i] = steps.inz
        return x, eps, nz, inz

    def bpd_columns(self, diffusion, nz, eps, proto):
        """nz.shape[0] columns of calc_bpd_loop, per column (:1617, then RAG.py:10-13): randn_like(x_start) in x_start's memory order
        (proto), then the pair.  Natively (ls_trng_randn continues torch's CPU stream per tensor and hands the advanced state back) when
        host_native allows it for a contiguous x_start; with torch's own calls otherwise.  Either way the generator ends where the
        reference's does."""
        native = host_native(diffusion, first_contiguous=proto.is_contiguous())
        if native < 0:
            for r in range(nz.shape[0]):
                nz[r].copy_(self.like(proto))
                self.pair_into(eps[r])
            return
        lib = _lib.load_library()
        st = th.get_rng_state()
        for r in range(nz.shape[0]):
            for dst in (nz[r], eps[r, 0], eps[r, 1]):
                rc = lib.ls_trng_randn(st.data_ptr(), st.numel(), dst.data_ptr(), dst.numel(), int(native), torch_rng.n_threads())
                if rc != 0:
                    raise _lib.EngineError(f"ls_trng_randn failed ({rc})")
        th.set_rng_state(st)


class _Steps:
    """The per-step draws of one p_sample_loop / ddim_sample_loop call of n_exec executed steps.

    p_sample / ddim_sample draw randn_like(x) (gaussian_diffusion.py:543/787).  x is the loop's start at the first executed step --
    the caller's ``noise``, strides included (``first``), when it was given with no init_image and no skip; contiguous otherwise -- but
    from then on it is the model-output-shaped view whose memory order is [T][B][J][F] (OutputProcess permutes, RAG.py:209-210), and
    randn_like preserves strides: the generator stream is consumed in MEMORY order through torch's non-contiguous path.
    ``inpainted``: the motion q_sample(inpainted_motion, t - 1) re-noises at the steps with t > 0 (:318); its draws land in ``inz``.
    ``diffusion``: whose native_host_rng switch decides (host_native) whether runs of steps are drawn natively."""

    def __init__(self, draws, shape, D, n_exec, first, inpainted, diffusion):
        self.draws, self.shape, self.D, self.n_exec = draws, tuple(shape), D, n_exec
        B, J, F, T = self.shape
        self.first_proto = draws._proto(first, self.shape)
        self.later_proto = th.empty(T, B, J, F, device=draws.rdev).permute(1, 2, 3, 0)
        self.inz = None
        if inpainted is not None:
            self.inz = th.zeros((n_exec,) + self.shape, device=draws.rdev)
            self.inp_proto = draws._proto(inpainted, self.shape)
        self.per_step_bytes = (2 * B * D + int(np.prod(self.shape))) * 4
        self.native = -1 if diffusion is None else host_native(diffusion, self.inz is not None, self.first_proto.is_contiguous())

    def buffers(self, n):
        """Unpinned (eps [n, 2, B, D], noise [n, B, J, F, T]) tapes on the generator's device."""
        return th.empty(n, 2, self.shape[0], self.D, device=self.draws.rdev), th.empty((n,) + self.shape, device=self.draws.rdev)

    def step(self, k, eps_k, nz_k):
        """Executed step k (t = n_exec - 1 - k), the reference's order: the model call's pair, the inpainting branch's draw, the step's
        own noise."""
        self.draws.pair_into(eps_k)
        if self.inz is not None and self.n_exec - 1 - k > 0:
            self.inz[k] = self.draws.like(self.inp_proto)
        nz_k.copy_(self.draws.like(self.first_proto if k == 0 else self.later_proto))

    def run(self, k0, eps_seg, nz_seg):
        """Steps k0 .. k0 + len(eps_seg) into (eps [n, 2, B, D], noise [n, B, J, F, T]): ONE native call for the run, or torch's calls
        step by step."""
        if self.native >= 0:
            torch_rng.fill_steps(eps_seg, nz_seg, k0 == 0, self.native)
        else:
            for r in range(eps_seg.shape[0]):
                self.step(k0 + r, eps_seg[r], nz_seg[r])
