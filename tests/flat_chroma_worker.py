"""Child process of the flat-chroma cases that depend on a setting the library reads once per process (RBT_PARSE_BANDS, RBT_ARENA_SHARE: the parent sets the
environment). argv[1]: "hostemu" or "gpu"; argv[2]: the case, a worker_* function of tests/flat_chroma_cases.py. Prints "OK <case>"."""
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rbt_lib
import flat_chroma_cases as F

R = rbt_lib.module()
ctx = R.Context(device=0) if sys.argv[1] == "gpu" else R.Context(lib_path=rbt_lib.HOSTEMU_LIB)
getattr(F, "worker_" + sys.argv[2])(ctx, R)
ctx.close()
print("OK", sys.argv[2])
