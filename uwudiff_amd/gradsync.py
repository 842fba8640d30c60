"""Data-parallel gradient exchange: one flat fp32 gradient buffer, one logical all-reduce per step.

The minibatch is sharded across ranks (one process per GPU; reference: Lightning DDP, commented
``devices: 4 / strategy: ddp`` in configs/demo_training.yaml:5-7, per-rank seed test_scripts/test_train.py:68-69).
Gradients are SUMMED over ranks here; the 1/world averaging is folded into the norm / AdamW kernels as
``pre_scale`` so no extra pass over the buffer is needed.

RCCL over xGMI is reached through ``torch.distributed`` (backend "nccl" == RCCL on ROCm).  The buffer is reduced
in a few large chunks on a dedicated communication stream; each chunk records an event, and the optimizer
kernel for chunk i waits only on event i, so AdamW on already-reduced chunks overlaps the reduction of the
rest (the mesh is point-to-point: 7 links x ~153 GB/s per GPU, so chunks are sized in the tens of MB, not the
25 MB DDP bucket default).  With gradient clipping the global norm needs every chunk first, so the optimizer
waits on the last event.  On CPU tensors (gloo, used by the tests) the same code runs synchronously.

Overlap with the backward pass: a model that can tell when a slice of its flat gradient is final (the DiT driver
records one event per group of transformer blocks, ``DiT.set_grad_ready_hook``) is attached with :meth:`attach`;
those slices (2/3 of DiT-S/2's gradient bytes) are reduced on the communication stream behind their event while the
rest of the backward still runs, and :meth:`all_reduce` afterwards only reduces what is left.  Every rank issues the
same collectives in the same order (block groups last-to-first, then the remainder in offset order).

Gradient accumulation (``Fitter(accumulate_grad_batches=N)``): inside a window the buffer holds a partial sum and nothing is
exchanged (:meth:`FlatGradSync.defer`); the batch that ends the window exchanges the whole sum once, as above.
"""
import ctypes
import os

import torch
import torch.distributed as dist


class _DirectRccl:
    """The C-ABI exchange (include/uwu_hip.h: uwu_comm_* / uwu_allreduce_flat): one RCCL communicator per rank created
    once; the 128-byte id travels through torch.distributed's broadcast.  Opt-in (UWU_RCCL_DIRECT=1)."""

    def __init__(self, device, group=None):
        from . import lib as L

        self.L = L
        rank, world = dist.get_rank(group), dist.get_world_size(group)
        idbuf = (ctypes.c_char * 128)()
        if rank == 0:
            L.call("uwu_comm_unique_id", ctypes.addressof(idbuf))
        t = torch.frombuffer(bytearray(idbuf.raw), dtype=torch.uint8).clone()
        t = t.to(device) if dist.get_backend(group) == "nccl" else t
        dist.broadcast(t, src=0, group=group)
        raw = bytes(t.cpu().tolist())
        self.comm = ctypes.c_void_p()
        with torch.cuda.device(device):
            L.call("uwu_comm_init", raw, rank, world, ctypes.byref(self.comm))

    def all_reduce(self, t, stream):
        # uwu_allreduce_flat takes a count of ncclFloat32 elements: anything else would silently reduce the wrong bytes.
        # UNVERIFIED at world > 1 (no multi-GPU box in the build loop; the world-1 identity test is all that ran): opt-in only.
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise TypeError(f"uwu_allreduce_flat reduces contiguous float32 slices (got {t.dtype}, contiguous={t.is_contiguous()})")
        self.L.call("uwu_allreduce_flat", self.comm, t.data_ptr(), t.numel(), stream.cuda_stream)


class FlatGradSync:
    def __init__(self, world_size=None, chunk_elems=8 * 1024 * 1024, group=None, single=False):
        """``single=True``: north_star's exchange as literally stated -- ONE all-reduce of the whole flat buffer after the
        backward (no early block-group reductions, no chunks), AdamW behind its one event.  The default overlaps: block
        groups are reduced from inside the backward and the rest in ``chunk_elems`` pieces.  Same object, same call sites,
        so the 8-GPU run can A/B the two (``bench.py --single-allreduce``)."""
        self.group = group
        self.single = bool(single)
        self.path = None  # which exchange ran last: "torch.distributed" | "uwu_allreduce_flat (direct RCCL)" (bench `comm.backend`)
        self.world = world_size if world_size is not None else (dist.get_world_size(group) if dist.is_initialized() else 1)
        self.chunk_elems = int(chunk_elems)
        self._comm_stream = None
        self._direct = None  # _DirectRccl when UWU_RCCL_DIRECT=1 (device tensors, world > 1)
        self.events = []
        self._early = []  # [(offset, length, event)] reduced from inside the backward of the current step
        self.deferred = False  # inside a gradient-accumulation window: the buffer holds a partial sum, nothing is exchanged

    @property
    def pre_scale(self):
        return 1.0 / self.world

    def chunks(self, n):
        c = n if self.single else self.chunk_elems
        return [(o, min(c, n - o)) for o in range(0, n, c)]

    def _stream(self, device):
        if self._comm_stream is None:
            self._comm_stream = torch.cuda.Stream(device=device)
        return self._comm_stream

    def _reduce(self, t, comm_stream):
        """Sum-all-reduce of a device slice on the communication stream (already current)."""
        if os.environ.get("UWU_RCCL_DIRECT", "0") == "1" and dist.get_backend(self.group) == "nccl":
            if self._direct is None:
                self._direct = _DirectRccl(t.device, self.group)
            self._direct.all_reduce(t, comm_stream)
            self.path = "uwu_allreduce_flat (direct RCCL communicator)"
        else:
            dist.all_reduce(t, op=dist.ReduceOp.SUM, group=self.group)
            self.path = f"torch.distributed/{dist.get_backend(self.group)}"

    def attach(self, model):
        """Reduce the slices ``model`` reports as final from inside its backward (no-op for one rank or for models
        without ``set_grad_ready_hook``).  Call once, after the model is on its device."""
        if self.world > 1 and not self.single and hasattr(model, "set_grad_ready_hook"):
            model.set_grad_ready_hook(self._on_ready)
        return self

    def defer(self, flag=True):
        """Gradient accumulation: while deferred the backward's ready slices are not reduced (:meth:`_on_ready` returns at once and
        records nothing) and :meth:`all_reduce` must not be called.  The batch that ends the window runs with ``defer(False)``:
        its backward and its :meth:`all_reduce` then exchange the whole accumulated sum once, exactly as a step without a window."""
        self.deferred = bool(flag)
        return self

    def _on_ready(self, flat_grad, ranges):
        """Called by the model between enqueueing its backward launches and returning to autograd."""
        if self.world == 1 or self.deferred:
            return
        if not flat_grad.is_cuda:  # gloo on CPU tensors (tests): synchronous
            for off, ln, _ in ranges:
                dist.all_reduce(flat_grad[off:off + ln], op=dist.ReduceOp.SUM, group=self.group)
                self._early.append((off, ln, None))
            return
        comm = self._stream(flat_grad.device)
        with torch.cuda.stream(comm):
            for off, ln, ready in ranges:
                comm.wait_event(ready)  # every gradient launch of this slice has completed
                self._reduce(flat_grad[off:off + ln], comm)
                ev = torch.cuda.Event()
                ev.record(comm)
                self._early.append((off, ln, ev))

    def all_reduce(self, flat_grad: torch.Tensor):
        """Launch the (chunked) sum-all-reduce of ``flat_grad`` in place -- of whatever :meth:`_on_ready` has not
        reduced already during this step's backward.  Returns the chunk list [(offset, length), ...] covering the whole
        buffer; on CUDA the work is asynchronous on the communication stream and ``self.events[i]`` marks chunk i
        reduced."""
        if self.deferred:
            raise RuntimeError("FlatGradSync.all_reduce inside a deferred (gradient accumulation) window: the partial sum would be "
                               "summed over the ranks now and again at the boundary")
        n = flat_grad.numel()
        early, self._early = sorted(self._early), []
        self.events = []
        if self.world == 1:
            return self.chunks(n)
        # the remainder: gaps between the early slices, cut into chunk_elems pieces
        rest, pos = [], 0
        for off, ln, _ in early + [(n, 0, None)]:
            while pos < off:
                step = off - pos if self.single else min(self.chunk_elems, off - pos)
                rest.append((pos, step))
                pos += step
            pos = max(pos, off + ln)
        chunks = []
        if flat_grad.is_cuda:
            comm = self._stream(flat_grad.device)
            comm.wait_stream(torch.cuda.current_stream(flat_grad.device))  # backward finished producing the buffer
            for off, ln, ev in early:  # already reduced (or about to be): the optimizer starts with these
                chunks.append((off, ln))
                self.events.append(ev)
            with torch.cuda.stream(comm):
                for off, ln in rest:
                    self._reduce(flat_grad[off:off + ln], comm)
                    ev = torch.cuda.Event()
                    ev.record(comm)
                    chunks.append((off, ln))
                    self.events.append(ev)
        else:
            chunks += [(off, ln) for off, ln, _ in early]
            for off, ln in rest:
                dist.all_reduce(flat_grad[off:off + ln], op=dist.ReduceOp.SUM, group=self.group)
                chunks.append((off, ln))
        return chunks

    def wait_chunk(self, i):
        if self.events:
            torch.cuda.current_stream().wait_event(self.events[i])

    def wait_all(self):
        for ev in self.events:
            torch.cuda.current_stream().wait_event(ev)


def shard_range(n_items, rank, world):
    """Contiguous shard [lo, hi) of ``n_items`` for ``rank`` (balanced, first ranks take the remainder)."""
    base, rem = divmod(n_items, world)
    lo = rank * base + min(rank, rem)
    return lo, lo + base + (1 if rank < rem else 0)
