// Stand-in declarations for cgltf.h: only the enums, struct fields and functions that the reference's
// model.h:301-460 touches.  ref_harness.cpp defines the three functions over a flattened copy of the glTF file that the
// tests write (tests/ref_harness.py).
#ifndef SRT_REFSHIM_CGLTF_H
#define SRT_REFSHIM_CGLTF_H
#include <cstddef>

typedef float cgltf_float;
typedef size_t cgltf_size;
typedef int cgltf_bool;

enum cgltf_file_type { cgltf_file_type_invalid, cgltf_file_type_gltf, cgltf_file_type_glb };
enum cgltf_result { cgltf_result_success, cgltf_result_file_not_found, cgltf_result_io_error, cgltf_result_invalid_json };
enum cgltf_attribute_type {
  cgltf_attribute_type_invalid, cgltf_attribute_type_position, cgltf_attribute_type_normal, cgltf_attribute_type_tangent,
  cgltf_attribute_type_texcoord, cgltf_attribute_type_color, cgltf_attribute_type_joints, cgltf_attribute_type_weights
};
enum cgltf_type {
  cgltf_type_invalid, cgltf_type_scalar, cgltf_type_vec2, cgltf_type_vec3, cgltf_type_vec4, cgltf_type_mat2,
  cgltf_type_mat3, cgltf_type_mat4
};
enum cgltf_primitive_type {
  cgltf_primitive_type_points, cgltf_primitive_type_lines, cgltf_primitive_type_line_loop, cgltf_primitive_type_line_strip,
  cgltf_primitive_type_triangles, cgltf_primitive_type_triangle_strip, cgltf_primitive_type_triangle_fan
};

struct cgltf_options { cgltf_file_type type; };
struct cgltf_buffer { void* data; cgltf_size size; };
struct cgltf_buffer_view { cgltf_buffer* buffer; cgltf_size offset; };
struct cgltf_accessor { cgltf_type type; cgltf_size count; cgltf_buffer_view* buffer_view; };
struct cgltf_attribute { cgltf_attribute_type type; cgltf_accessor* data; };
struct cgltf_image { char* uri; };
struct cgltf_texture { cgltf_image* image; };
struct cgltf_texture_view { cgltf_texture* texture; };
struct cgltf_pbr_metallic_roughness {
  cgltf_texture_view base_color_texture;
  cgltf_texture_view metallic_roughness_texture;
  cgltf_float base_color_factor[4];
  cgltf_float metallic_factor;
  cgltf_float roughness_factor;
};
struct cgltf_material {
  cgltf_bool has_pbr_metallic_roughness;
  cgltf_pbr_metallic_roughness pbr_metallic_roughness;
  cgltf_texture_view normal_texture;
};
struct cgltf_primitive {
  cgltf_primitive_type type;
  cgltf_accessor* indices;
  cgltf_material* material;
  cgltf_attribute* attributes;
  cgltf_size attributes_count;
};
struct cgltf_mesh { cgltf_primitive* primitives; cgltf_size primitives_count; };
struct cgltf_data { cgltf_mesh* meshes; cgltf_size meshes_count; void* owner; };

cgltf_result cgltf_parse_file(const cgltf_options* options, const char* path, cgltf_data** out_data);
cgltf_result cgltf_load_buffers(const cgltf_options* options, cgltf_data* data, const char* gltf_path);
void cgltf_free(cgltf_data* data);
#endif
