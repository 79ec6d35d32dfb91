"""Worker of tests/test_gpu_hw_queues.py: started with GPU_MAX_HW_QUEUES=4 in its environment (what a launcher may have put there). Creating the first context must write the
library's own request over it (dev_init, before this process's first HIP call); the value is read back through libc's getenv - os.environ is a copy made when Python
started. Then one small GOF is transcoded and compared with the oracle's bytes. argv[1]: the value expected. Prints "ok <value>"."""
import ctypes
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import oracle_lib as O
import parity_cases as PC
import rbt_lib

libc = ctypes.CDLL(None)
libc.getenv.restype = ctypes.c_char_p
libc.getenv.argtypes = [ctypes.c_char_p]
assert libc.getenv(b"GPU_MAX_HW_QUEUES") == b"4", "the worker must start with the launcher's value"
R = rbt_lib.module()
ctx = R.Context(device=0)
got = libc.getenv(b"GPU_MAX_HW_QUEUES")
assert got == sys.argv[1].encode(), (got, sys.argv[1])
streams, _ = PC.r5_gof(128, 128, 1, 61)
ps = PC.r3_params(R)
outs = ctx.transcode_gof(streams, ps)
want = O.transcode_data(streams, [(p.video_type, p.qp, p.occupancy_precision, p.log2_ctb, p.ctb_rows_per_slice, p.md5_sei, p.occupancy_rd) for p in ps])
assert outs == want, "transcode differs from the oracle"
ctx.close()
print("ok", got.decode())
