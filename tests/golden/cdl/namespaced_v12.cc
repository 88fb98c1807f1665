<?xml version="1.0" encoding="UTF-8"?>
<ColorCorrection xmlns="urn:ASC:CDL:v1.2" id="ns_1">
  <SOPNode>
    <Slope>1.2 1.0 0.8</Slope>
    <Offset>0.1 0.0 -0.1</Offset>
    <Power>1.0 1.5 2.0</Power>
  </SOPNode>
  <SatNode>
    <Saturation>1.25</Saturation>
  </SatNode>
</ColorCorrection>
