"""One process per GPU without torch in the process.

`python -m torch.distributed.run --nproc-per-node N bench.py ...` (or any launcher that sets RANK / WORLD_SIZE / LOCAL_RANK) starts the
ranks; each rank renders its tiles with its own mcpt_device and the frames are gathered into rank 0's HBM over an RCCL communicator
that the ranks build themselves (mcpt_comm_*, csrc/proc_comm.cpp).  torch is deliberately NOT imported: a process that imports torch
runs libmcpt.so's kernels on the wheel's bundled HIP runtime instead of the release they were compiled against, and the
library refuses that since version 105.  What the ranks need from a launcher is only their rank, the world size and a way to pass
RCCL's 128-byte unique id from rank 0 to the others -- a file in the node's temporary directory, named after the launcher's process id
(all ranks are children of one launcher process) and the rendezvous port, written atomically by rank 0 and polled by the others.  A
record belongs to one attempt of one launch (exchange_id): ranks that took ids of different launches would wait in ncclCommInitRank
for each other, and that call has no time limit.

The torch.distributed form of the same partition / gather is dist.py (kept for the gloo rehearsal on CPU and as `--launcher torch`)."""
import ctypes as C
import os
import tempfile
import time

import numpy as np

from ._lib import RenderParams, check, lib

ID_BYTES = 128


def launch_env():
    """(rank, world, local_rank) from the launcher's environment"""
    return int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("LOCAL_RANK", os.environ.get("RANK", "0")))


def rendezvous_file(tag=None):
    """where rank 0 leaves the unique id: one name per launch (the ranks share their parent, the launcher)"""
    if tag is None:
        tag = os.environ.get("MCPT_RDZV_TAG") or "%d_%s" % (os.getppid(), os.environ.get("MASTER_PORT", "0"))
    return os.path.join(os.environ.get("MCPT_RDZV_DIR") or tempfile.gettempdir(), "mcpt_rdzv_%s" % tag)


def launch_key():
    """what tells one attempt of a launch from another under the same launcher process: torch.distributed.run's run id and restart
    count (a --max-restarts respawn keeps the launcher, its process id and the port, and counts up); empty under other launchers"""
    run, restart = os.environ.get("TORCHELASTIC_RUN_ID"), os.environ.get("TORCHELASTIC_RESTART_COUNT")
    if run is None and restart is None:
        return b""
    return ("%s/%s" % (run or "", restart or "")).encode()


def launch_began(pid=None):
    """when the launcher process (default: this process's parent) started, as time.time() counts, from /proc: field 22 of
    /proc/<pid>/stat is the start in clock ticks after boot, /proc/uptime the seconds since boot.  Rounded UP by the resolution of the
    two (a tick, 10 ms) and a little more: a record has to be younger than this to be taken, and no rank writes one within 50 ms of
    its launcher's start.  None where /proc does not say, or says a time that has not come yet."""
    try:
        with open("/proc/%d/stat" % (os.getppid() if pid is None else pid)) as fh:
            ticks = int(fh.read().rsplit(")", 1)[1].split()[19])           # (the command name may hold blanks: count from its ")")
        with open("/proc/uptime") as fh:
            uptime = float(fh.read().split()[0])
        now = time.time()
        began = now - (uptime - ticks / os.sysconf("SC_CLK_TCK"))
        # (a /proc whose uptime is not the clock the ticks count in -- some container file systems rewrite it -- gives a start in the future)
        return began + 0.05 if began <= now else None
    except (OSError, ValueError, IndexError):
        return None


def exchange_id(rank, world, make_id, path=None, timeout=120.0, started=None, began=None):
    """rank 0: make_id() -> bytes, published; other ranks: wait for it.  A record belongs to one attempt of one launch: it carries
    rank 0's clock and launch_key(), and a reader takes it only if the key is its own and the stamp is not older than `began`, the
    start of the launcher process (launch_began(); given explicitly by tests).  So a file left behind under the same name -- by a
    crashed or timed-out launch whose process id and port a container hands out again, or by the previous attempt of a launcher that
    respawns its ranks -- is never returned, however recent; the reader waits for rank 0 to replace it and raises after `timeout`.
    The ranks of a launch start at different times, so a rank's own start (`started`) bounds less: a record more than 300 s older
    than it is not taken either, and where /proc does not give the launcher's start that is the only bound."""
    path = path or rendezvous_file()
    started = time.time() if started is None else started
    if world == 1:
        return make_id()
    key = launch_key()
    if rank == 0:
        ident = make_id()
        assert len(ident) == ID_BYTES
        tmp = "%s.%d.tmp" % (path, os.getpid())
        with open(tmp, "wb") as fh:
            fh.write(np.float64(time.time()).tobytes() + ident + key)
        os.replace(tmp, path)                      # atomic: a reader sees nothing or everything
        return ident
    if began is None:
        began = launch_began()
    floor = started - 300.0 if began is None else max(began, started - 300.0)
    deadline = time.time() + timeout
    while time.time() < deadline:
        try:
            with open(path, "rb") as fh:
                raw = fh.read()
        except OSError:
            raw = b""
        if len(raw) >= 8 + ID_BYTES and raw[8 + ID_BYTES:] == key and float(np.frombuffer(raw[:8], dtype=np.float64)[0]) >= floor:
            return raw[8:8 + ID_BYTES]
        time.sleep(0.02)
    raise TimeoutError("rank %d: no unique id from rank 0 under %s within %.0f s" % (rank, path, timeout))


class ProcessGroup:
    """The ranks of one launch: RCCL communicator over xGMI, gather of the frame into rank 0, barrier, small all-reduce."""

    def __init__(self, ordinal, rank=None, world=None, rdzv_path=None, started=None):
        env_rank, env_world, _ = launch_env()
        self.rank = env_rank if rank is None else rank
        self.world = env_world if world is None else world
        self.ordinal = ordinal
        self._path = rdzv_path or rendezvous_file()

        def make_id():
            buf = (C.c_uint8 * ID_BYTES)()
            n = lib().mcpt_comm_unique_id(buf, ID_BYTES)
            if n != ID_BYTES:
                check(n if n < 0 else -3)
            return bytes(buf)
        ident = exchange_id(self.rank, self.world, make_id, self._path, started=started)
        self._h = C.c_void_p()
        arr = (C.c_uint8 * ID_BYTES).from_buffer_copy(ident)
        check(lib().mcpt_comm_create(ordinal, self.rank, self.world, arr, ID_BYTES, C.byref(self._h)))

    def size(self):
        return lib().mcpt_comm_size(self._h)

    def gather_frame(self, scene, d_frame_ptr, tile_w=0, tile_h=0, stream=None):
        rp = RenderParams(spp=1, seed=0, rank=self.rank, world=self.world, tile_w=tile_w, tile_h=tile_h, flags=0)
        check(lib().mcpt_comm_gather_frame(self._h, scene._h, C.byref(rp), C.c_void_p(d_frame_ptr), stream))

    def allreduce(self, values, op="sum"):
        v = np.ascontiguousarray(values, dtype=np.float64).copy()
        assert v.size <= 64
        check(lib().mcpt_comm_allreduce(self._h, v.ctypes.data_as(C.POINTER(C.c_double)), v.size, 0 if op == "sum" else 1))
        return v

    def barrier(self):
        check(lib().mcpt_comm_allreduce(self._h, None, 0, 0))

    def close(self):
        if getattr(self, "_h", None):
            lib().mcpt_comm_free(self._h)
            self._h = None
            if self.rank == 0 and self.world > 1:
                try:
                    os.remove(self._path)
                except OSError:
                    pass

    def __del__(self):
        try:
            self.close()
        except Exception:       # interpreter shutdown
            pass
