// unit8_table.h -- T[k] = (float) k / 255.0f, evaluated by the compiler with IEEE division: the values uint8 / 255.0 has on
// the host (quantize8 of color.hip, the fused picture of roi.hip).  Include inside the file's anonymous namespace.
struct Unit8Table {
    float v[256];
};
constexpr Unit8Table make_unit8() {
    Unit8Table t{};
    for (int k = 0; k < 256; ++k) t.v[k] = (float)k / 255.0f;
    return t;
}
__device__ const Unit8Table kUnit8 = make_unit8();
