// LDS-DMA (__builtin_amdgcn_global_load_lds) in the convolution and MBConv families (conv_tile.hpp, mbconv_tile.hpp): its operand
// types, and the zero-initialised page that padded pixels, padded taps and rows past the end are fetched from.  ``static``: the
// library is built without relocatable device code, so a __device__ symbol is visible to the kernels of its own file only -- every
// file that includes this header has its own 256-byte page.
#pragma once
#include "common.hpp"

typedef __attribute__((address_space(1))) const void* gptr_t;
typedef __attribute__((address_space(3))) void* lptr_t;
static __device__ __attribute__((aligned(256))) float ocv_zero_page[64];
