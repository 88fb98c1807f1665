<?xml version="1.0" encoding="UTF-8"?>
<ColorCorrection id="shot_010">
  <SOPNode>
    <Description>warm up, lift blue</Description>
    <Slope>1.3 1.25 1.1</Slope>
    <Offset>-0.08 0.0 0.05</Offset>
    <Power>0.8 1.0 1.2</Power>
  </SOPNode>
  <SatNode>
    <Saturation>0.6</Saturation>
  </SatNode>
</ColorCorrection>
