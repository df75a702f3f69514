// Stand-in for stb_image_write.h: the hot-path headers include it and call nothing from it.
