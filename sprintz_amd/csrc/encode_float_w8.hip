// encode_float_w8.hip -- the encoders on a float source (quant.h), 8-bit elements.
#include "../../include/sprintz_mi355x.h"
#include "launch.h"
SPRINTZ_ENCODE_FLOAT_UNIT(8)
