#include <hip/hip_runtime.h> /* the reference kernel files name the runtime header only; they call nothing of it by a cuda* name */
