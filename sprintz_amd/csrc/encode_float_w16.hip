// encode_float_w16.hip -- the encoders on a float source (quant.h), 16-bit elements.
#include "../../include/sprintz_mi355x.h"
#include "launch.h"
SPRINTZ_ENCODE_FLOAT_UNIT(16)
