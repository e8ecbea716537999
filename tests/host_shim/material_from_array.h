// TEST INFRASTRUCTURE ONLY.  The flat 29-float material of the oracle's known-answer hooks (layout: oracle/oracle_pt.h) as the
// device headers' PbrMaterial, in the fixed shading frame T = (1, 0, 0), B = (0, 1, 0), N = Ng = Nc = (0, 0, 1).  One definition for
// the host compile of the headers (tests/host_shim/device_on_host.cpp) and for the device compile (tests/device_kat/kat_device.hip),
// so that both are fed the same material as oracle_pt.cpp's materialFromArray.  Include after pt_bsdf.h / pt_shading.h.
#pragma once

namespace pt {
PT_DEV PbrMaterial materialFromArray(const float* m)
{
  PbrMaterial p = defaultPbrMaterial();
  p.baseColor = mk3(m[0], m[1], m[2]);
  p.roughness = mk2(m[3], m[4]);
  p.metallic  = m[5];
  p.ior1 = m[6]; p.ior2 = m[7];
  p.specular = m[8];
  p.specularColor = mk3(m[9], m[10], m[11]);
  p.transmission = m[12];
  p.thickness = m[13];
  p.clearcoat = m[14]; p.clearcoatRoughness = m[15];
  p.sheenColor = mk3(m[16], m[17], m[18]); p.sheenRoughness = m[19];
  p.iridescence = m[20]; p.iridescenceIor = m[21]; p.iridescenceThickness = m[22];
  p.diffuseTransmissionFactor = m[23];
  p.diffuseTransmissionColor = mk3(m[24], m[25], m[26]);
  p.dispersion = m[27];
  p.retroreflection = m[28];
  p.N = p.Ng = p.Nc = mk3(0, 0, 1);
  p.T = mk3(1, 0, 0);
  p.B = mk3(0, 1, 0);
  return p;
}
}  // namespace pt
