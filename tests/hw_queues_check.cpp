// TEST-ONLY (tests/test_hw_queues.py): prints what rbtk::hw_queues_wanted (csrc/rbt_kernels.h) makes of RBT_HW_QUEUES, once with the variable unset and then for every
// argument as its value, one number per line.
#include <cstdio>
#include <cstdlib>
#include "../rabbit-transcoding_amd/csrc/rbt_kernels.h"

int main(int argc, char** argv) {
  unsetenv("RBT_HW_QUEUES");
  printf("%d\n", rbtk::hw_queues_wanted(getenv("RBT_HW_QUEUES")));
  for (int i = 1; i < argc; i++) { setenv("RBT_HW_QUEUES", argv[i], 1); printf("%d\n", rbtk::hw_queues_wanted(getenv("RBT_HW_QUEUES"))); }
  return 0;
}
