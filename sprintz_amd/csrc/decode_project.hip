// decode_project.hip -- the project-rows unit (launch.h: SPRINTZ_ROW_OP_UNIT): decode_fast on its one-column-a-lane mappings for the shapes whose
// projected block is whole 16-byte pieces, the generic kernel for everything else.  decode_uni.h is not taught the mode: its shapes go to the
// generic kernel.
#include "launch.h"
SPRINTZ_ROW_OP_UNIT(project, sprintz::kQueryProject, SPRINTZ_DISPATCH_DECODE_FAST_LANES_1)
