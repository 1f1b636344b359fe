"""float64 numpy restatement of the flat optimiser's contract (include/wsdl_hip.h, "flat optimiser") - the oracle of
csrc/flat_optim.hip, beside augment_oracle.py.

Three algorithms on ONE flat buffer - Adam + L2 (torch.optim.Adam(weight_decay=)), AdamW (torch.optim.AdamW), SGD with momentum
(torch.optim.SGD, dampening 0) - preceded by torch.nn.utils.clip_grad_norm_ on the grad_scale-averaged gradient and by the
non-finite skip (torch: ``optimizer.step()`` is simply not called).  tests/test_flat_optim.py holds it against live torch in
float64; the GPU tests hold the kernels against it.
"""
import numpy as np

ADAM_L2, ADAMW, SGD = 0, 1, 2
BLOCK = 64                  # floats per entry of a decay table


def f32(x):
    """A hyper-parameter as the kernels read it: rounded to float32 (hyper_dev holds floats), then exact in float64.  The
    kernels run the algorithm ON those values - beta2 = float32(0.999) is 0.99900001287, so 1 - beta2 differs from 0.001 by
    1.3e-5 of itself - and an oracle that is to bound their ARITHMETIC has to start from the same inputs, as it does for the
    parameters and gradients.  None stays None; a pair is rounded element-wise."""
    if x is None:
        return None
    if isinstance(x, (tuple, list)):
        return tuple(f32(v) for v in x)
    return float(np.float32(x))


def total_norm(g, grad_scale=1.0):
    """Norm of the averaged gradient, every square taken in float64."""
    g = np.asarray(g, dtype=np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        return abs(float(grad_scale)) * float(np.sqrt(np.sum(g * g)))


def clip_coef(norm, max_norm):
    """torch.nn.utils.clip_grad_norm_: min(1, max_norm / (norm + 1e-6)); no clipping without max_norm."""
    if not max_norm:
        return 1.0
    c = max_norm / (norm + 1e-6)
    return c if (c < 1.0 or c != c) else 1.0


def expand_blocks(table, n):
    """Per-element decay mask (bool, n) from a per-64-floats table; None: decay everywhere."""
    if table is None:
        return np.ones(n, dtype=bool)
    return np.repeat(np.asarray(table).astype(bool), BLOCK)[:n]


class FlatOracle:
    @classmethod
    def as_kernel_reads(cls, algo, p, **kw):
        """The oracle on the float32 values of the hyper-parameters (``f32``): what the device comparisons use."""
        kw.setdefault("betas", (0.9, 0.999))
        kw.setdefault("eps", 1e-8)
        for name in ("lr", "betas", "eps", "weight_decay", "momentum", "grad_scale", "max_norm"):
            if name in kw:
                kw[name] = f32(kw[name])
        return cls(algo, p, **kw)

    def __init__(self, algo, p, *, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, momentum=0.0, nesterov=False,
                 grad_scale=1.0, max_norm=None, skip_nonfinite=False, decay_blocks=None):
        self.algo = algo
        self.p = np.array(p, dtype=np.float64)
        self.m = np.zeros_like(self.p)
        self.v = np.zeros_like(self.p)
        self.lr, self.betas, self.eps, self.wd = lr, betas, eps, weight_decay
        self.mu, self.nesterov, self.grad_scale = momentum, nesterov, grad_scale
        self.max_norm, self.skip_nonfinite = max_norm, skip_nonfinite
        self.decays = expand_blocks(decay_blocks, self.p.size)
        self.step_no = 0            # steps that were applied (what the bias corrections see)
        self.skipped = 0
        self.norm = self.clip = None

    def step(self, g):
        """One step on gradient ``g``; returns False when the step was skipped (``norm`` / ``clip``: what it measured)."""
        g = np.asarray(g, dtype=np.float64)
        use_norm = self.max_norm is not None or self.skip_nonfinite
        self.norm = total_norm(g, self.grad_scale) if use_norm else None
        # the contract judges the norm as the float it reports: finite in double but above FLT_MAX is inf there, and skipped
        with np.errstate(over="ignore"):
            reported = np.float32(self.norm) if use_norm else None
        if self.skip_nonfinite and not np.isfinite(reported):
            self.skipped += 1
            self.clip = clip_coef(self.norm, self.max_norm)
            return False
        self.clip = clip_coef(self.norm, self.max_norm) if use_norm else 1.0
        self.step_no += 1
        with np.errstate(over="ignore", invalid="ignore"):
            g = g * (self.grad_scale * self.clip)
            wd = np.where(self.decays, self.wd, 0.0)
            if self.algo == SGD:
                g = g + wd * self.p
                if self.mu != 0:
                    self.m = self.mu * self.m + g
                    g = g + self.mu * self.m if self.nesterov else self.m
                self.p = self.p - self.lr * g
                return True
            b1, b2 = self.betas
            if self.algo == ADAMW:
                self.p = self.p * (1.0 - self.lr * wd)
            else:
                g = g + wd * self.p
            self.m = self.m + (g - self.m) * (1.0 - b1)
            self.v = self.v * b2 + (1.0 - b2) * g * g
            bc1, bc2 = 1.0 - b1 ** self.step_no, 1.0 - b2 ** self.step_no
            denom = np.sqrt(self.v) / np.sqrt(bc2) + self.eps
            self.p = self.p - (self.lr / bc1) * (self.m / denom)
        return True
