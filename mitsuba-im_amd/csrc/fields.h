// fields.h -- launch arguments of the field stage (kernels_field.hip), shared with api.cpp.  The field list travels to the kernels BY VALUE, so every
// per-field branch is wave-uniform; nothing is added to Queues or DScene.
#pragma once
#include <stdint.h>
#include "../../include/mi355pt.h"

#define MI_MAX_FIELDS 8
struct FieldArgs {
    uint32_t n;                        // fields requested (1..MI_MAX_FIELDS)
    uint32_t needs;                    // bit k: some field has kind k (albedo and relPosition are evaluated only where asked for)
    uint32_t kind[MI_MAX_FIELDS];      // MI_FIELD_*
    float undefined[MI_MAX_FIELDS][3]; // value of a camera ray that leaves the scene
    float w2c[12];                     // rows 0..2 of the inverse of the sensor's world transform (relPosition)
    const int32_t *tri_shape;          // [n_tris] shape index of every triangle, -1 for members of a shape group (shapeIndex only, else null)
    uint32_t n_meshes;                 // analytic shape i has shape index n_meshes + i
    // prevPosition / motion (filled before every launch, mi_scene_mark_frame): the scene's state at the last mark.  Null tables: the scene was never marked
    // (or was committed again since), previous = current
    const float *prev_pos;             // [n_verts * 3] the vertex array at the mark, shape-group members included (gathered through TriShade::i0..i2)
    const float *prev_inst;            // [n_instances * 12] rows 0..2 of every instance's to_world at the mark
    float m_cur[12], m_prev[12];       // world -> pixel rows X, Y, W (mi_scene_world_to_pixel) of the camera as it is / as it was at the mark
    float o_cur[3], o_prev[3];         // camera origin now / at the mark
};
