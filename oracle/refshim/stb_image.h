// Stand-in declaration for stb_image.h: the one function the reference's texture.h:62,115 calls.
// ref_harness.cpp defines it over raw files that the tests decode with PIL.
#ifndef SRT_REFSHIM_STB_IMAGE_H
#define SRT_REFSHIM_STB_IMAGE_H
typedef unsigned char stbi_uc;
stbi_uc* stbi_load(char const* filename, int* x, int* y, int* channels_in_file, int desired_channels);
#endif
